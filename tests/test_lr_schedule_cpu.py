"""The learning-rate schedule (include/ff_hip_lr.h) without a GPU: the formula against a float64 numpy restatement, the host route on the tiny
golden DLRM over the CPU oracle, compile()'s refusals (each names its flag) and the driver's pass-through and start-up line."""
import os
import subprocess
import sys

import numpy as np
import pytest

import dlrm_helpers as H
import lr_helpers as LH
from dlrm_flexflow_amd import capi, ffmodel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def backend(oracle):
    return H.oracle_backend()


@pytest.mark.parametrize("sched", [(0, 0, 0), (3, 0, 0), (2, 3, 3), (4, 4, 1), (0, 2, 4000), (5, 5, 0)], ids=str)
@pytest.mark.parametrize("base", [0.01, 1.0, 3e-4])
def test_formula_equals_the_float64_restatement(backend, sched, base):
    W, S, N = sched
    for k in range(S + N + 6):
        got, want = ffmodel.lr_schedule_value(k, base, W, S, N), LH.schedule_f32(k, base, W, S, N)
        assert np.float32(got).tobytes() == np.float32(want).tobytes(), (k, got, want)
    if sched == (0, 0, 0):
        assert all(ffmodel.lr_schedule_value(k, base) == float(np.float32(base)) for k in range(4))


def test_the_floor_binds(backend):
    # r = 1/4000 at the last decay step: 3e-4 * r^2 = 1.9e-11 < 1e-7
    W, S, N, base = 0, 2, 4000, 3e-4
    floor = float(np.float32(1e-7))
    assert ffmodel.lr_schedule_value(S + N - 1, base, W, S, N) == floor
    assert ffmodel.lr_schedule_value(S + N + 100, base, W, S, N) == floor            # held
    assert ffmodel.lr_schedule_value(S + 10, base, W, S, N) > floor
    assert LH.schedule_f64(S + N - 1, base, W, S, N) == 1e-7


def test_header_list_matches_prototypes_and_the_oracle_has_no_lr_extension(oracle):
    syms = capi.lr_header_symbols()
    assert len(syms) == len(set(syms)) and set(syms) == set(capi._SIGS_LR)
    assert capi.lr_header_abi_version() >= 1
    with pytest.raises(capi.FFHError):
        capi.lr_api(oracle.lib())
    # ff_hip.h's own list is untouched by the extension
    assert not set(syms) & set(capi.header_symbols())


def test_hip_library_exports_the_lr_extension():
    from dlrm_flexflow_amd import build
    out = subprocess.check_output(["nm", "-D", "--defined-only", build.build_hip()], text=True)
    exp = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert not [s for s in capi.lr_header_symbols() if s not in exp]


def test_host_route_follows_the_formula_and_equals_constant_rate_steps(backend):
    """(2,3,3), 8 steps on the host route: current_lr() is the formula before every step, and after each step the weights are those of a model
    driven to that point with a FRESH constant-rate optimizer per step set to that step's value (rebuilt from the previous step's weights)."""
    sched, steps, base = (2, 3, 3), 8, 0.01
    run = LH.run_model(backend, steps, sched, device_lr=None, optimizer=("sgd", base), per_step_state=True)
    assert run["route"] == 1 and run["lr_steps"] == steps and not run["uses_graph"]
    want = [LH.schedule_f32(k, base, *sched) for k in range(steps)]
    assert run["lrs"] == want
    assert len(set(want)) == 4           # warm-up, plateau, decay and the held value all occur
    prev = None
    for k in range(steps):
        m, h = LH.build(backend, (0, 0, 0), None, optimizer=("sgd", want[k]))
        assert m.counter("lr_route") == 0
        if prev is not None:
            for name, li in h["names"].items():
                m.parameter(li, 0).set_weights(prev[f"{name}.weight"])
                if not name.startswith("emb"):
                    m.parameter(li, 1).set_weights(prev[f"{name}.bias"])
        LH.step(m)
        ref = LH.params(m, h)
        for name in ref:
            assert np.array_equal(ref[name], run["states"][k][name]), (k, name)
        prev = ref


def test_zero_schedule_is_bit_identical_to_no_flags(backend):
    a = LH.run_model(backend, 4, (0, 0, 0), device_lr=None)
    m, h = LH.build(backend, (0, 0, 0), None, flags=["--lr-num-warmup-steps", "0", "--lr-decay-start-step=0", "--lr-num-decay-steps", "0"])
    assert m.counter("lr_route") == 0
    for _ in range(4):
        LH.step(m)
    b = LH.params(m, h)
    for k in a["state"]:
        assert np.array_equal(a["state"][k], b[k]), k
    golden = H.run_steps(H.build_golden_dlrm(backend)[0], H.build_golden_dlrm(backend)[1], steps=1)      # (the fixture still builds without flags)
    assert golden


def test_adam_on_the_host_route_uses_the_scheduled_alpha(backend):
    sched, base = (2, 3, 3), 0.01
    run = LH.run_model(backend, 5, sched, device_lr=None, flags=["--sparse-embedding-optimizer"], optimizer=("adam", base))
    assert run["route"] == 1 and run["lrs"] == [LH.schedule_f32(k, base, *sched) for k in range(5)]
    const = LH.run_model(backend, 5, (0, 0, 0), device_lr=None, flags=["--sparse-embedding-optimizer"], optimizer=("adam", base))
    assert any(not np.array_equal(run["state"][k], const["state"][k]) for k in run["state"])


_REFUSALS = {
    "decay_inside_warmup": (["--lr-num-warmup-steps", "5", "--lr-decay-start-step", "3", "--lr-num-decay-steps", "2"], "--lr-decay-start-step"),
    "negative_warmup": (["--lr-num-warmup-steps", "-1"], "--lr-num-warmup-steps"),
    "negative_start": (["--lr-decay-start-step=-2"], "--lr-decay-start-step"),
    "negative_steps": (["--lr-num-decay-steps", "-3"], "--lr-num-decay-steps"),
    "device_lr_without_extension": (["--device-lr"], "--device-lr"),
}
_CHILD = """
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import lr_helpers as LH
LH.build({backend!r}, (0, 0, 0), None, flags={flags!r})
print("compiled")
"""


@pytest.mark.parametrize("case", list(_REFUSALS))
def test_compile_refuses_and_names_the_flag(backend, case):
    flags, named = _REFUSALS[case]
    code = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), backend=backend, flags=flags)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "compiled" not in r.stdout, r.stdout
    fatal = [l for l in r.stderr.splitlines() if "FATAL" in l]
    assert fatal and named in fatal[0], r.stderr[-600:]


def test_run_dlrm_passes_the_flags_through_and_prints_the_route(backend):
    args = ["--backend", backend] + H.DOT_ARGS + ["--epochs", "1", "--lr", "0.02", "--lr-num-warmup-steps", "2", "--lr-decay-start-step=3",
                                                  "--lr-num-decay-steps", "3"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "dlrm_flexflow_amd", "run_dlrm.py"), *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-800:]
    line = [l for l in r.stdout.splitlines() if l.startswith("[DLRM] lr schedule:")]
    assert len(line) == 1, r.stdout[-800:]
    assert "W=2" in line[0] and "S=3" in line[0] and "N=3" in line[0] and "route=host" in line[0] and "0.02" in line[0]
    assert "THROUGHPUT" in r.stdout
    # without the flags the line is not printed
    r = subprocess.run([sys.executable, os.path.join(ROOT, "dlrm_flexflow_amd", "run_dlrm.py"), "--backend", backend, *H.DOT_ARGS, "--epochs", "1"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "lr schedule" not in r.stdout
