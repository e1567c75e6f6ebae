"""The body of k_sim_joint_stops (csrc/sim_joint_stops.h) on the CPU: tests/kernels/sim_joint_stops_host.cpp includes the kernel's header as it is,
runs the lanes one after the other and is built here as a stand-alone program under the address and undefined-behaviour sanitizers.  Without fused
multiply-adds (-ffp-contract=off) its arithmetic is the mirror's, so what the dynamics would integrate and the state rows after every step equal
``joint_stops.step`` bit for bit: on the 20 imposed states of tests/test_gpu_sim_joint_stops.py, and on a tree of 150 actuated joints, where the
loop beyond 64 lanes runs and an index out of a part of the row would be the sanitizer's to find."""
import os
import subprocess

import numpy as np
import pytest

from mpc_benchmark_amd import joint_stops as js
from tests import test_gpu_sim_joint_stops as gpu_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = gpu_cases.B


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("joint_stops_host") / "sim_joint_stops_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", out,
                    os.path.join(ROOT, "tests", "kernels", "sim_joint_stops_host.cpp")], check=True)
    return out


def _robot_case():
    rb = gpu_cases._sim_robot()
    x = np.tile(rb.x0, (B, 1))
    lo, hi = gpu_cases._tables(rb, x)
    return rb.model.nq, rb.model.nv, lo, hi, gpu_cases._effort(rb), gpu_cases._designed_states(rb, x)


def _wide_case(nu=150, steps=20):
    """random ranges and states; robot 0 without limits, every 7th joint of robot 3 seized"""
    rng = np.random.default_rng(3)
    lo = np.tile(rng.uniform(-1.0, 0.0, nu), (B, 1))
    hi = lo + rng.uniform(0.0, 1.0, (B, nu))
    lo[0], hi[0] = -np.inf, np.inf
    hi[3, ::7] = lo[3, ::7]
    return nu + 7, nu + 6, lo, hi, rng.uniform(1.0, 100.0, nu), rng.normal(size=(steps, B, 2 * nu + 13))


@pytest.mark.parametrize("case", [_robot_case, _wide_case])
def test_the_kernel_body_on_the_host_equals_the_mirror_bit_for_bit(program, tmp_path, case):
    nq, nv, lo, hi, scale, xs = case()
    nu, S = nv - 6, len(xs)
    taus = np.random.default_rng(1).normal(size=(S, B, nu)) * 5.0
    taus[0, 0, 0] = -0.0   # (an idle joint keeps even the sign of a zero: the torque is copied, not added to)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        np.array([B, nu, nq, nv, S], dtype=np.int32).tofile(f)
        for a in (gpu_cases.ROWS, lo, hi, scale):
            np.ascontiguousarray(a, dtype=float).tofile(f)
        for x, t in zip(xs, taus):
            np.ascontiguousarray(x).tofile(f)
            np.ascontiguousarray(t).tofile(f)
    subprocess.run([program, fin, fout], check=True)
    got = np.fromfile(fout).reshape(S, -1)
    state = js.reset(B, nu)
    acted = 0
    for s in range(S):
        tau_stop = js.step(state, gpu_cases.ROWS, lo, hi, xs[s][:, 7:nq], xs[s][:, nq + 6:], scale)
        assert np.array_equal(got[s, :B * nu].reshape(B, nu), js.integrated(taus[s], tau_stop)), s
        assert np.array_equal(got[s, B * nu:].reshape(B, -1), state), s
        acted += int((tau_stop != 0.0).sum())
    assert acted > S * nu and np.signbit(got[0, 0])
