"""Every hand-built boundary call of tests/matcher_boundary_cases.py through pkg.Matcher: kernel == oracle == stated expectation
(match arrays, assign / occupied, counts, best_idx / best_dist), integer and bit equality only.  The two tracking searches also
go through SearchByProjection(_last)_batch_device with cap = number of features."""
import numpy as np
import pytest

import matcher_boundary_cases as mbc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(mbc.CALLS))
def test_boundary_call_kernel_equals_oracle_equals_expectation(pkg, oracle, name):
    call = mbc.CALLS[name]()
    want = mbc.expected(call)
    mbc.assert_same(mbc.run(call, mbc.oracle_backend(oracle)), want, "oracle vs stated expectation")
    mbc.assert_same(mbc.run(call, mbc.KernelBackend(pkg)), want, "kernel vs stated expectation")


def _device_calls():
    """the calls of the two tracking searches that the device-resident entries can take: monocular frames, no level window"""
    out = []
    for n in sorted(mbc.CALLS):
        c = mbc.CALLS[n]()
        if c["search"] in ("mp", "last") and "u_right" not in c["args"]["g"] and not c["params"].get("level_window", 0):
            out.append(n)
    return out


@pytest.mark.parametrize("name", _device_calls())
def test_boundary_call_through_the_device_batch_entries(pkg, name):
    call = mbc.CALLS[name]()
    mbc.assert_same(mbc.run(call, mbc.DeviceBatchBackend(pkg)), mbc.expected(call), "device batch entry vs stated expectation")
