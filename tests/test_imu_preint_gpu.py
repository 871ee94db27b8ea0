"""IMU pre-integration on the GPU (include/orbslam3_hip_imu_preint.h) against tests/imu_preint_reference.py.

States and prediction: every output block is held to truth (long double) within 4 x budget + 4 x 2^-24, the budget being the largest
error of the three float32 variants of the reference over the cases of the same length; it is computed when the test runs
(imu_preint_cases.reference_data, shared) and printed with the device's figure (run with -s).  tests/test_imu_preint_reference.py
says where the rule comes from and prints the budgets.  info9: relative Frobenius error against mpmath at 60 digits on the device's own
float C within 100 kappa_2(C9) 2^-53, on the cases with 2 measurements or more.  Everything else is bitwise: the interpolation loop
against its float32 restatement, host entry against device entry, a job alone against the same job among 70, seven measurements at
once against three and then four, two equal calls, untouched states, the Initialize state, the measurement count.

The device's own figures (MI355X; every test prints them next to budget and bound): the largest share of a bound is 0.35 (JRg after
400 measurements: 1.28e-6, budget 8.6e-7, bound 3.68e-6; C9 there 3.99e-6 of 1.57e-5); JRg / JVg / JPg after 2 and 3 measurements 5e-8 ..
1.6e-7 where the budgets are 3e-6 .. 6e-6; the prediction at or below its budgets (twb2 1.15e-6 of 4.8e-6 at 400); info9 5e-16 .. 3.3e-15
against bounds of 1.7e-12 (65 measurements) .. 1.8e-9 (2), the crafted clamp state 2.2e-15."""
import ctypes as C
import importlib

import numpy as np
import pytest

import imu_preint_cases as cases
import imu_preint_reference as ref

pytestmark = pytest.mark.gpu
NAMES = list(cases.CASES)
ERR_ARG = -3


@pytest.fixture(scope="module")
def capi(pkg):
    return importlib.import_module("orb_slam3-1_amd.capi")


@pytest.fixture(scope="module")
def pre(pkg):
    p = pkg.ImuPreintegrator()
    yield p
    p.close()


@pytest.fixture(scope="module")
def torch_(pkg):
    import torch
    return torch


@pytest.fixture(scope="module")
def device_states(capi, pre):
    """every case in ONE call of the host entry; the last state is named by no job"""
    states, jobs, meas = cases.pack(capi, NAMES, extra_states=1)
    states["C"] = 7.0                                                           # what a reset has to clear
    states["dT"] = 3.0
    before = states[-1].copy()
    st = pre.preintegrate(states, jobs, meas)
    assert not st.any()
    assert states[-1].tobytes() == before.tobytes(), "a state named by no job changed"
    assert states["n_meas"][:-1].tolist() == [cases.CASES[n]["n"] for n in NAMES]
    assert np.array_equal(states["b"][:-1], jobs["bias"]) and np.array_equal(states["bu"][:-1], jobs["bias"])
    states.setflags(write=False)
    return states


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _back(t, dtype):
    return t.cpu().numpy().view(dtype)


def _same(a, b):
    return a.tobytes() == b.tobytes()


@pytest.mark.parametrize("n", cases.LENGTHS)
def test_states_within_budget(device_states, n):
    for name in cases.cases_of_length(n):
        s = device_states[NAMES.index(name)]
        cases.check_against_truth(name, ref.blocks(s), ref.BLOCKS)
        assert ref.zero_blocks_are_zero(s["C"]), "a zero block of C is not exactly zero"


def test_prediction_within_budget(capi, pre, device_states):
    out, st = pre.predict(np.array(device_states), cases.predict_jobs(capi, NAMES))
    assert not st.any()
    for i, name in enumerate(NAMES):
        cases.check_against_truth(name, out[i], ref.PREDICTED)


def test_links(capi, pre, device_states):
    """the physical cases, the crafted clamp state and a state with C = 0 in one call"""
    i7 = NAMES.index("n7_a")
    zero = capi.imu_state_new(1, cases.NGA, cases.NGA_WALK)
    states = np.concatenate([device_states[:-1], cases.clamp_state(capi, device_states[i7])[None], zero])
    n = len(states)
    spec = np.zeros(n, capi.IMU_LINK_SPEC_DTYPE)
    spec["state"] = np.arange(n)
    spec["walk_state"] = np.arange(n)
    spec["walk_state"][-1] = -1
    spec["walk_state"][0] = -1
    spec["kf1"], spec["kf2"] = np.arange(n) + 3, np.arange(n) * 2 + 1
    spec["info_scale"] = 1e-2
    spec["robust"] = np.arange(n) % 2
    links, st = pre.links(states, spec)
    assert st[:-1].tolist() == [0] * (n - 1) and st[-1] == ERR_ARG, st          # C = 0 has no inverse; the other links are not affected
    assert np.array_equal(links["kf1"], spec["kf1"]) and np.array_equal(links["kf2"], spec["kf2"]) and np.array_equal(links["robust"], spec["robust"])
    for k in ("dR", "dV", "dP", "JRg", "JVg", "JVa", "JPg", "JPa", "dT"):
        assert _same(np.ascontiguousarray(links[k]), np.ascontiguousarray(states[k])), k
    assert _same(np.ascontiguousarray(links["bias0"]), np.ascontiguousarray(states["b"]))
    assert np.isfinite(links["info9"]).all() and not links["info_gyro"][0].any() and not links["info_acc"][-1].any()
    for i, name in enumerate(NAMES):
        if cases.CASES[name]["n"] < 2:
            continue                                                            # one measurement: C9 has rank 6, only finite values and status 0 are asked
        e, lim = ref.rel_frobenius(links[i]["info9"], ref.info9_truth(states[i]["C"], 1e-2)), ref.info9_bound(states[i]["C"])
        print("%-8s info9 device %.2e  bound %.2e" % (name, e, lim))
        assert e <= lim, (name, e, lim)
        assert np.array_equal(links[i]["info9"], links[i]["info9"].T)
    for i in range(1, n - 1):
        g, a = ref.walk_info(states[i]["C"])
        d = np.eye(3, dtype=bool)
        for got, want in ((links[i]["info_gyro"], g), (links[i]["info_acc"], a)):
            assert not got[~d].any() and np.abs(got[d] / want[d] - 1).max() <= 1e-14
    crafted, t = links[n - 2]["info9"], ref.info9_truth(states[n - 2]["C"], 1e-2)
    keep = np.arange(9) != 8
    assert not crafted[8, :].any() and not crafted[:, 8].any(), "the clamped axis did not come back exactly zero"
    e, lim = ref.rel_frobenius(crafted[np.ix_(keep, keep)], t[np.ix_(keep, keep)]), ref.info9_bound(states[i7]["C"])
    print("crafted  info9 device %.2e  bound %.2e" % (e, lim))
    assert not t[8, :].any() and e <= lim


def _streams(capi):
    streams = cases.frame_streams()
    cap = 8
    smp = np.zeros((len(streams), cap), capi.IMU_DTYPE)
    for b, s in enumerate(streams):
        k = len(s["ts"])
        smp["ts"][b, :k], smp["gyro"][b, :k], smp["acce"][b, :k] = s["ts"], s["gyro"], s["acce"]
    n_imu = np.array([len(s["ts"]) for s in streams], np.int32)
    tp, tc = np.array([s["t_prev"] for s in streams], np.int64), np.array([s["t_cur"] for s in streams], np.int64)
    return streams, smp, n_imu, tp, tc


def test_frame_measurements_bitwise(capi, pre, torch_):
    streams, smp, n_imu, tp, tc = _streams(capi)
    meas, cnt = pre.frame_measurements(smp, n_imu, tp, tc)
    assert cnt.tolist() == [0, 0, 1, 2, 7]
    for b, s in enumerate(streams):
        a, w, dt = ref.frame_measurements(s["ts"], s["gyro"], s["acce"], s["t_prev"], s["t_cur"])
        k = cnt[b]
        assert _same(np.ascontiguousarray(meas["a"][b, :k]), a) and _same(np.ascontiguousarray(meas["w"][b, :k]), w) and _same(np.ascontiguousarray(meas["dt"][b, :k]), dt)
    # the device entry writes the same bits
    B, cap = smp.shape
    d_smp, d_n, d_tp, d_tc = _dev(torch_, smp), _dev(torch_, n_imu), _dev(torch_, tp), _dev(torch_, tc)
    d_meas, d_cnt = _dev(torch_, np.zeros((B, cap), capi.IMU_MEAS_DTYPE)), _dev(torch_, np.full(B, 9, np.int32))
    pre.frame_measurements_device(d_smp.data_ptr(), d_n.data_ptr(), d_tp.data_ptr(), d_tc.data_ptr(), B, cap, d_meas.data_ptr(), d_cnt.data_ptr(),
                                  torch_.cuda.current_stream().cuda_stream)
    torch_.cuda.synchronize()
    m2, c2 = _back(d_meas, capi.IMU_MEAS_DTYPE).reshape(B, cap), _back(d_cnt, np.int32)
    assert np.array_equal(c2, cnt)
    for b in range(B):
        assert _same(m2[b, :cnt[b]], meas[b, :cnt[b]])


def test_host_entry_equals_device_entry(capi, pre, torch_, device_states):
    states, jobs, meas = cases.pack(capi, NAMES, extra_states=1)
    states["C"] = 7.0
    states["dT"] = 3.0
    d_s, d_j, d_m, d_st = _dev(torch_, states), _dev(torch_, jobs), _dev(torch_, meas), _dev(torch_, np.full(len(jobs), 9, np.int32))
    s = torch_.cuda.current_stream().cuda_stream
    pre.preintegrate_device(d_s.data_ptr(), len(states), d_j.data_ptr(), len(jobs), d_m.data_ptr(), len(meas), d_st.data_ptr(), s)
    # links and prediction from the states in HBM, without a trip to the host
    spec = np.zeros(len(NAMES), capi.IMU_LINK_SPEC_DTYPE)
    spec["state"] = spec["walk_state"] = np.arange(len(NAMES))
    spec["info_scale"] = 1.0
    pj = cases.predict_jobs(capi, NAMES)
    d_spec, d_links, d_lst = _dev(torch_, spec), _dev(torch_, np.zeros(len(spec), capi.LIBA_LINK_DTYPE)), _dev(torch_, np.full(len(spec), 9, np.int32))
    d_pj, d_po, d_pst = _dev(torch_, pj), _dev(torch_, np.zeros(len(pj), capi.IMU_PREDICT_OUT_DTYPE)), _dev(torch_, np.full(len(pj), 9, np.int32))
    pre.links_device(d_s.data_ptr(), len(states), d_spec.data_ptr(), len(spec), d_links.data_ptr(), d_lst.data_ptr(), s)
    pre.predict_device(d_s.data_ptr(), len(states), d_pj.data_ptr(), len(pj), d_po.data_ptr(), d_pst.data_ptr(), s)
    torch_.cuda.synchronize()
    assert not _back(d_st, np.int32).any() and not _back(d_lst, np.int32).any() and not _back(d_pst, np.int32).any()
    assert _same(_back(d_s, capi.IMU_STATE_DTYPE), device_states)
    links, lst = pre.links(np.array(device_states), spec)
    out, pst = pre.predict(np.array(device_states), pj)
    assert _same(_back(d_links, capi.LIBA_LINK_DTYPE), links) and _same(_back(d_po, capi.IMU_PREDICT_OUT_DTYPE), out)


def test_results_do_not_depend_on_the_batch(capi, pre, device_states):
    """a job alone, the same job among 70, and the same call twice"""
    name = "n65_a"
    i = NAMES.index(name)
    s1, j1, m1 = cases.pack(capi, [name])
    assert not pre.preintegrate(s1, j1, m1).any()
    assert _same(s1[0], device_states[i])
    s1b, _, _ = cases.pack(capi, [name])
    assert not pre.preintegrate(s1b, j1, m1).any() and _same(s1b, s1)
    c = cases.make_case(name)
    rng = np.random.default_rng(3)
    states = capi.imu_state_new(70, cases.NGA, cases.NGA_WALK)
    jobs = np.zeros(70, capi.IMU_JOB_DTYPE)
    meas = np.zeros(70 * 65, capi.IMU_MEAS_DTYPE)
    meas["a"], meas["w"], meas["dt"] = rng.normal(0, 3, (len(meas), 3)), rng.normal(0, 0.4, (len(meas), 3)), cases.DT
    for j in range(70):
        jobs[j] = (69 - j, 65 * j, 1 + (7 * j) % 65, 1, rng.normal(0, 0.02, 6))
    jobs[41] = (5, 65 * 41, 65, 1, c["bias"])                                   # the case, in the second wave, writing state 5
    jobs[64] = (28, 65 * 64, jobs[64]["count"], 1, jobs[64]["bias"])            # (job 64 wrote state 5)
    meas[65 * 41:65 * 42] = m1
    assert len(set(jobs["state"].tolist())) == 70
    assert not pre.preintegrate(states, jobs, meas).any()
    assert _same(states[5], s1[0])


def test_three_then_four_equals_seven(capi, pre, device_states):
    for name in ("n7_a", "slow7"):
        s, j, m = cases.pack(capi, [name])
        j["count"] = 3
        assert not pre.preintegrate(s, j, m).any() and s["n_meas"][0] == 3
        j[0] = (0, 3, 4, 0, np.full(6, np.nan))                                 # continuing: the bias of the job is not read
        assert not pre.preintegrate(s, j, m).any() and s["n_meas"][0] == 7
        assert _same(s[0], device_states[NAMES.index(name)])


def test_reset_without_measurements_is_initialize(capi, pre):
    s = capi.imu_state_new(2, cases.NGA, cases.NGA_WALK)
    for k in ("dT", "b", "bu", "dR", "dV", "dP", "JRg", "JVg", "JVa", "JPg", "JPa", "avgA", "avgW", "C"):
        s[k] = 5.0
    s["n_meas"] = 12
    bias = np.arange(1, 7, dtype=np.float32) / 64
    jobs = np.zeros(1, capi.IMU_JOB_DTYPE)
    jobs[0] = (1, 0, 0, 1, bias)
    assert not pre.preintegrate(s, jobs, np.zeros(0, capi.IMU_MEAS_DTYPE)).any()
    want = capi.imu_state_new(1, cases.NGA, cases.NGA_WALK)[0]
    want["b"] = want["bu"] = bias
    assert _same(s[1], want) and s["dT"][0] == 5.0 and s["n_meas"][0] == 12


def test_device_entry_reports_bad_contents_per_job(capi, pre, torch_):
    """state index out of range, a range past the measurements, two writers of one state, a NaN, dt = 0: ORBX_ERR_ARG in d_status[job],
    that state untouched, the good job of the call done, and the handle usable afterwards"""
    s, j1, m = cases.pack(capi, ["n7_a"], extra_states=4)
    good = s.copy()
    assert not pre.preintegrate(good, j1, m).any()
    meas = np.concatenate([m, m[:2], m[:2]])
    meas["a"][8, 1] = np.nan
    meas["dt"][10] = 0.0
    jobs = np.zeros(7, capi.IMU_JOB_DTYPE)
    b = j1[0]["bias"]
    jobs[0] = (0, 0, 7, 1, b)
    jobs[1] = (5, 0, 7, 1, b)           # no such state
    jobs[2] = (1, 3, 9, 1, b)           # 3 + 9 > 11 measurements
    jobs[3] = (2, 0, 2, 1, b)           # two writers of state 2
    jobs[4] = (2, 2, 2, 1, b)
    jobs[5] = (3, 7, 2, 1, b)           # a NaN
    jobs[6] = (4, 9, 2, 1, b)           # dt = 0
    s["dT"] = 3.0
    before = s.copy()
    d_s, d_j, d_m, d_st = _dev(torch_, s), _dev(torch_, jobs), _dev(torch_, meas), _dev(torch_, np.full(7, 9, np.int32))
    pre.preintegrate_device(d_s.data_ptr(), len(s), d_j.data_ptr(), 7, d_m.data_ptr(), len(meas), d_st.data_ptr(), torch_.cuda.current_stream().cuda_stream)
    torch_.cuda.synchronize()
    assert _back(d_st, np.int32).tolist() == [0] + [ERR_ARG] * 6
    after = _back(d_s, capi.IMU_STATE_DTYPE)
    assert _same(after[1:], before[1:]) and _same(after[0], good[0])
    with pytest.raises(capi.OrbxError):                                         # the host entry refuses the same call as a whole ...
        pre.preintegrate(s.copy(), jobs, meas)
    again = cases.pack(capi, ["n7_a"], extra_states=4)[0]
    assert not pre.preintegrate(again, j1, m).any() and _same(again, good)      # ... and the handle is still usable
