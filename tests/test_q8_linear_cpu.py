"""int8 Linear layers for evaluation (include/ffh_q8_linear.h, --eval-mlp-dtype int8) without a GPU: the header against the bindings, the export,
the flag, every refusal of compile() on the CPU oracle (which lacks the extension, so the flag refusals are shown to come first), the numpy rule."""
import os
import subprocess

import numpy as np
import pytest

from dlrm_flexflow_amd import build, capi, ffmodel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "dlrm_flexflow_amd", "host", "dlrm_testing")
SMALL = ["-b", "64", "--arch-sparse-feature-size", "8", "--arch-embedding-size", "100-200-50", "--arch-mlp-bot", "13-16-8",
         "--arch-mlp-top", "32-16-1", "--data-size", "512", "--epochs", "1"]
FLAG = "--eval-mlp-dtype"
EVAL = ["--eval-batches", "2"]


@pytest.fixture(scope="module", autouse=True)
def _built():
    build.build_host()


def _driver(*extra):
    import dlrm_helpers as H
    return subprocess.run([EXE, "--backend", H.oracle_backend(), *SMALL, *extra], capture_output=True, text=True, timeout=300)


def test_header_list_equals_the_bindings_and_the_library_exports_it():
    ext = capi.EXTENSIONS["q8_linear"]
    syms = ext.header_symbols()
    assert syms == list(capi._SIGS_Q8_LINEAR) and ext.header_abi_version() == 1 and not hasattr(capi, "Q8_LINEAR_HEADER_PATH")
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.HIP_LIB_PATH], text=True)
    assert all(f" T {s}\n" in out for s in syms)


@pytest.mark.parametrize("spelling", [(FLAG, "fp32"), (FLAG + "=fp32",)], ids=["two-tokens", "one-token"])
def test_both_spellings_are_taken(spelling):
    r = _driver(*spelling)
    assert r.returncode == 0 and "eval MLP" not in r.stdout, r.stderr[-2000:]


def test_unknown_value_is_refused_naming_both():
    r = _driver(FLAG + "=int4")
    assert r.returncode != 0 and f"{FLAG} int4: 'fp32' or 'int8'" in r.stderr, r.stderr[-2000:]
    with pytest.raises(ValueError, match="'fp32' or 'int8'"):
        ffmodel.FFConfig(argv=["-b", "16"]).set(eval_mlp_dtype="int4")


@pytest.mark.parametrize("extra,words", [
    ([FLAG, "int8"], ["--eval-batches", "drop --eval-mlp-dtype int8"]),
    ([FLAG + "=int8", *EVAL, "--allow-tensor-op-math-conversion"], ["drop --allow-tensor-op-math-conversion"]),
    ([FLAG, "int8", *EVAL, "--fp32-split-bf16x3"], ["drop --fp32-split-bf16x3"]),
    ([FLAG, "int8", *EVAL], ["without the q8-linear extension", "include/ffh_q8_linear.h", "drop --eval-mlp-dtype int8"]),
], ids=["no-evaluation", "tensor-op", "split", "library"])
def test_compile_refusals_name_the_flag_to_drop(extra, words):
    r = _driver(*extra)
    assert r.returncode != 0 and "THROUGHPUT" not in r.stdout
    assert all(w in r.stderr for w in words) and ("extension" in r.stderr) == ("extension" in " ".join(words)), r.stderr[-2000:]


def test_the_numpy_rule_on_three_rows():
    v = np.array([[0.0, -0.0, 0.0, 0.0],                   # a row of zeros: scale 0, codes 0
                  [1.0, -4.0, 2.0, 0.5],                   # a negative extreme: inv = 31.75 -> 31.75, -127, 63.5, 15.875
                  [127.0, 2.5, -3.5, 0.49]], np.float32)   # inv = 1: ties to even both ways
    q, s = ffmodel.q8_linear_quantize_reference(v)
    assert q.dtype == np.int8 and q.tolist() == [[0, 0, 0, 0], [32, -127, 64, 16], [127, 2, -4, 0]]
    assert s.dtype == np.float32 and s.tolist() == [0.0, float(np.float32(4.0) / np.float32(127.0)), 1.0]
    x, W, b = v[1:], v, np.float32([0.5, -1.0, 2.0])
    acc = q[1:].astype(np.int64) @ q.astype(np.int64).T
    want = (acc.astype(np.float32) * (s[1:, None] * s[None, :])) + b
    assert np.array_equal(ffmodel.q8_linear_reference(x, W, b), want)
    assert np.array_equal(ffmodel.q8_linear_reference(x, W, b, capi.AC_MODE_RELU), np.maximum(want, 0))
