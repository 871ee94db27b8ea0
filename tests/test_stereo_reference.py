"""The numpy restatement of Frame::ComputeStereoMatches (tests/stereo_reference.py, written from reference src/Frame.cc:931-1101)
against the C++ oracle: two independent statements of the operation must give the same floats, on the hand-built boundary cases
(tests/stereo_boundary_cases.py, whose import already checked the stated outcome codes) and on two synthetic frames with the
oracle extractor's own key points.  CPU only."""
import numpy as np
import pytest

import stereo_boundary_cases as bc
import stereo_reference as ref
from oracle_api import oracle_stereo_matches


@pytest.mark.parametrize("name", list(bc.CASES))
def test_restatement_equals_oracle_on_boundary_case(name):
    c = bc.CASES[name]
    want = bc.reference(name)
    exL, exR = bc.oracle_extractors(c["geom"], c["sheet"])
    n, ur, dp = oracle_stereo_matches(exL, exR, c["kps_l"], c["desc_l"], c["kps_r"], c["desc_r"], c["mb"], c["mbf"])
    if c["off_level"]:
        assert n == -2              # the documented contract: the oracle gives up where cv::Mat::rowRange / colRange would assert
        return
    assert n == want["n_matches"]
    np.testing.assert_array_equal(ur, want["u_right"])
    np.testing.assert_array_equal(dp, want["depth"])
    assert ur.dtype == want["u_right"].dtype == np.float32
    assert ((want["u_right"] >= 0) == np.isin(want["code"], (ref.ACCEPTED, ref.ACCEPTED_CLAMPED))).all()


def test_every_outcome_and_topic_is_covered():
    assert all(len(v) >= 2 for v in bc.OUTCOME_TABLE.values()), bc.OUTCOME_TABLE
    assert set(bc.TOPICS) >= {"row_band", "octave_window", "disparity_window", "descriptor_gate", "first_minimum", "rounding", "right_edge",
                              "best_shift", "parabola", "final_gate", "median", "entry"}
    assert [bc.reference(n)["uncut"]["code"].shape[0] for n in bc.MEDIAN_CASES] == list(bc.MEDIAN_SIZES)


@pytest.mark.parametrize("seed,nfeat,mb,mbf", [(0, 1000, 0.11, 47.9), (2, 2000, 0.06, 25.0)])
def test_restatement_equals_oracle_on_synthetic_frame(oracle, synth, seed, nfeat, mb, mbf):
    left, right = synth.make_stereo_pair(seed)
    oL, oR = oracle.extractor(nfeat, 1.2, 8, 20, 7), oracle.extractor(nfeat, 1.2, 8, 20, 7)
    _, kL, dL = oL.extract(left, (0, 0)); _, kR, dR = oR.extract(right, (0, 0))
    n0, ur0, dp0 = oracle_stereo_matches(oL, oR, kL, dL, kR, dR, mb, mbf)
    t = oL.tables()
    r = ref.stereo_matches([oL.level_image(l) for l in range(8)], [oR.level_image(l) for l in range(8)], t["scale"], t["inv_scale"],
                           kL, dL, kR, dR, mb, mbf)
    assert n0 == r["n_matches"] > 0.3 * len(kL)
    np.testing.assert_array_equal(r["u_right"], ur0)
    np.testing.assert_array_equal(r["depth"], dp0)
    assert (r["code"] == ref.CUT_BY_MEDIAN).any() and (r["code"] == ref.ACCEPTED).sum() > 0.2 * len(kL)
