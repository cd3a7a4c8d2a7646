"""8-bit embedding rows for evaluation (include/ff_hip_q8.h, --eval-embedding-dtype int8) without a GPU: the numpy restatement of the rule and
the byte layout, the header and the bindings, the flag, and every refusal of compile() with the flag to drop -- on the CPU oracle, which does
not export the extension, so each refusal is shown to come before the library checks."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import q8_helpers as Q
from dlrm_flexflow_amd import build, capi, ffmodel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "dlrm_flexflow_amd", "host", "dlrm_testing")
LAUNCHER = os.path.join(ROOT, "dlrm_flexflow_amd", "run_dlrm.py")
HOST_LIB = os.path.join(ROOT, "dlrm_flexflow_amd", "host", "libffmodel.so")
SMALL = ["-b", "64", "--arch-sparse-feature-size", "8", "--arch-embedding-size", "100-200-50", "--arch-mlp-bot", "13-16-8",
         "--arch-mlp-top", "32-16-1", "--data-size", "512", "--epochs", "1"]
FLAG = "--eval-embedding-dtype"


@pytest.fixture(scope="module", autouse=True)
def _built():
    build.build_host()


def _oracle():
    import dlrm_helpers as H
    return H.oracle_backend()


def _driver(*extra, small=SMALL):
    return subprocess.run([EXE, "--backend", _oracle(), *small, *extra], capture_output=True, text=True, timeout=300)


# ---- the rule and the layout -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mag", [1e-30, 1e-20, 1e-8, 1e-3, 1.0, 1e3, 1e20, 1e30])
def test_codes_span_0_to_255_at_every_magnitude(mag):
    rng = np.random.default_rng(7)
    w = (rng.standard_normal((50, 64)) * mag).astype(np.float32)
    codes, scale, bias = ffmodel.q8_quantize_reference(w)
    wide = ((w - bias[:, None]) * (np.float32(255.0) / ((w.max(1) - bias) + np.float32(1e-8)))[:, None])
    assert codes.dtype == np.uint8 and wide.min() >= 0.0 and np.rint(wide).max() <= 255.0       # nothing wrapped in the cast
    assert np.all(codes.min(1) == 0)
    if mag >= 1e-3:
        assert np.all(codes.max(1) == 255)
    deq = ffmodel.q8_dequantize_reference(codes, scale, bias)
    rng_ = w.max(1) - w.min(1)
    assert np.all(np.abs(deq - w) <= (rng_ / 255.0 * 0.5 * 1.01 + np.abs(w).max(1) * 2.0 ** -22)[:, None] + (1e-8 if mag < 1e-3 else 0.0))


def test_constant_and_negative_zero_rows_are_exact():
    w = np.stack([np.full(16, 0.3, np.float32), np.full(16, -0.0, np.float32), np.full(16, -7.25e10, np.float32)])
    codes, scale, bias = ffmodel.q8_quantize_reference(w)
    assert not codes.any() and not scale[0] and not scale[2]
    deq = ffmodel.q8_dequantize_reference(codes, scale, bias)
    assert np.array_equal(deq[0], w[0]) and np.array_equal(deq[2], w[2])
    assert np.all(deq[1].view(np.uint32) == 0) and bias[1].view(np.uint32) == 0                 # -0 row: bias +0, every element +0


def test_the_rule_is_idempotent():
    """Quantizing a dequantized row reproduces its codes -- for every row whose range is far above the 1e-8 in `inv` (random rows, the outlier,
    1e30) or so far below it that every code is 0 (constant, -0, 1e-30).  A range near 1e-8 is the exception by construction: the 1e-8 holds
    the codes below 255 (a range of 5e-9 tops out at 85), the dequantized row's range is then a third of the first, and its codes shrink again."""
    rng = np.random.default_rng(11)
    for D in (4, 16, 128, 260):
        w = Q.make_table(rng, 300, D)
        span = w.max(1) - w.min(1)
        keep = (span > 1e-3) | (span < 1e-20)
        assert 0 < (~keep).sum() < 10                               # the table holds such a row, and little else is left out
        codes, scale, bias = ffmodel.q8_quantize_reference(w[keep])
        again, _, _ = ffmodel.q8_quantize_reference(ffmodel.q8_dequantize_reference(codes, scale, bias))
        assert np.array_equal(again, codes), D


def test_two_roundings_are_not_an_fma():
    """The contract names a multiply and then an add; the fused form differs on a large share of elements (so a kernel must not contract)."""
    rng = np.random.default_rng(3)
    codes, scale, bias = ffmodel.q8_quantize_reference(rng.standard_normal((200, 64)).astype(np.float32))
    two = ffmodel.q8_dequantize_reference(codes, scale, bias)
    fma = (codes.astype(np.float64) * scale[:, None].astype(np.float64) + bias[:, None].astype(np.float64)).astype(np.float32)
    assert 0.2 < np.mean(two != fma) < 0.9


def test_byte_layout_round_trips():
    rng = np.random.default_rng(5)
    for D in (4, 16, 260):
        w = Q.make_table(rng, 37, D)
        codes, scale, bias = ffmodel.q8_quantize_reference(w)
        for rb in (D + 8, Q.row_bytes_for(D, True), D + 40):
            rows = ffmodel.q8_pack_rows(codes, scale, bias, rb)
            assert rows.shape == (37, rb) and rows.dtype == np.uint8
            assert np.array_equal(rows[:, :D], codes) and not rows[:, D + 8:].any()
            assert np.array_equal(rows[:, D:D + 4].copy().view("<f4").reshape(-1).view(np.uint32), scale.view(np.uint32))
            assert np.array_equal(rows[:, D + 4:D + 8].copy().view("<f4").reshape(-1).view(np.uint32), bias.view(np.uint32))
            c2, s2, b2 = ffmodel.q8_unpack_rows(rows, D)
            assert np.array_equal(c2, codes) and np.array_equal(s2.view(np.uint32), scale.view(np.uint32)) and np.array_equal(b2.view(np.uint32), bias.view(np.uint32))
    assert ffmodel.q8_pack_rows(codes, scale, bias).shape[1] == D + 8                           # the default: fbgemm's layout
    for bad in (D + 4, D + 10):
        with pytest.raises(ValueError):
            ffmodel.q8_pack_rows(codes, scale, bias, bad)


# ---- the header and the bindings -------------------------------------------------------------------------------------------------------
def test_header_list_abi_version_and_prototypes_agree():
    syms = capi.q8_header_symbols()
    assert syms and len(syms) == len(set(syms)) and set(syms) == set(capi._SIGS_Q8)
    assert capi.q8_header_abi_version() >= 1
    body = open(capi.Q8_HEADER_PATH).read().split("#define FFH_Q8_API_LIST")[0]
    for s in syms:
        assert body.count(s + "(") == 1, s


def test_struct_sizes_match_a_c_compiler(tmp_path):
    assert ctypes.sizeof(capi.EmbTableQ8) == 48 and ctypes.sizeof(capi.Q8Source) == 40
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ff_hip_q8.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", sizeof(ffh_emb_table_q8), '
                   'offsetof(ffh_emb_table_q8, row_bytes), sizeof(ffh_q8_source), offsetof(ffh_q8_source, bf16)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [48, capi.EmbTableQ8.row_bytes.offset, 40, capi.Q8Source.bf16.offset]


def test_the_oracle_does_not_export_the_extension(oracle):
    lib = capi.FFHLib(oracle.ORACLE_LIB)
    with pytest.raises(capi.FFHError, match="no q8 extension"):
        capi.q8_api(lib)


def test_the_two_copies_of_the_lane_geometry_are_one_text():
    """RowLanes stays in embedding_fwd.hip (tests/test_stream_cap_cpu.py reads it there) and embedding_q8.hip carries a copy: the same struct, to the byte."""
    import re
    csrc = os.path.join(ROOT, "dlrm_flexflow_amd", "csrc")
    body = lambda f: re.search(r"^struct RowLanes \{.*?^\};$", open(os.path.join(csrc, f)).read(), re.S | re.M).group(0)
    a, b = body("embedding_fwd.hip"), body("embedding_q8.hip")
    assert a == b and "block_rows(int U) const { return 4LL * rpw * U; }" in a


def test_quantizer_rows_per_trip_formula():
    assert [capi.Q8Api.quantize_rows_per_trip(D) for D in (4, 8, 12, 16, 128, 256, 260, 1024, 1040)] == [256, 128, 64, 256, 32, 16, 4, 4, 4]


def test_c_api_exports_the_setter():
    out = subprocess.check_output(["nm", "-D", "--defined-only", HOST_LIB], text=True)
    assert " flexflow_config_set_eval_embedding_dtype" in out
    assert "flexflow_config_set_eval_embedding_dtype" in open(os.path.join(ROOT, "dlrm_flexflow_amd", "host", "ffmodel_c.h")).read()


# ---- the flag and the refusals ---------------------------------------------------------------------------------------------------------
def test_default_and_fp32_leave_the_run_as_it_was():
    base = _driver()
    assert base.returncode == 0, base.stderr[-2000:]
    for flags in ((FLAG, "fp32"), (FLAG + "=fp32",)):
        r = _driver(*flags)
        assert r.returncode == 0, r.stderr[-2000:]
        assert "eval tables" not in r.stdout and "eval tables" not in base.stdout
        pick = lambda out: [l for l in out.splitlines() if l.startswith("[DLRM]") or "loss" in l]
        assert pick(r.stdout) == pick(base.stdout)


@pytest.mark.parametrize("value", ["int4", "", "INT8"])
def test_unknown_value_is_refused(value):
    r = _driver(f"{FLAG}={value}")
    assert r.returncode != 0 and f"{FLAG} {value}: 'fp32' or 'int8'" in r.stderr, r.stderr[-2000:]


def test_python_config_takes_the_field():
    c = ffmodel.FFConfig(argv=["-b", "16"], backend=_oracle())
    assert c.set(eval_embedding_dtype="int8") is c and c.set(eval_embedding_dtype="fp32") is c
    with pytest.raises(ValueError, match="'fp32' or 'int8'"):
        c.set(eval_embedding_dtype="int4")


@pytest.mark.parametrize("spelling", [(FLAG, "int8"), (FLAG + "=int8",)], ids=["two-tokens", "one-token"])
def test_int8_without_evaluation_is_refused(spelling):
    r = _driver(*spelling)
    assert r.returncode != 0 and "THROUGHPUT" not in r.stdout
    assert FLAG + " int8" in r.stderr and "--eval-batches" in r.stderr and "extension" not in r.stderr, r.stderr[-2000:]


D6 = ["-b", "64", "--arch-sparse-feature-size", "6", "--arch-embedding-size", "100-200-50", "--arch-mlp-bot", "13-16-6",
      "--arch-mlp-top", "24-16-1", "--data-size", "512", "--epochs", "1"]


# tables of 8 columns behind a bottom MLP of 6: the first table's rows start at column 6 of the 30-column Concat buffer
BOT6 = ["-b", "64", "--arch-sparse-feature-size", "8", "--arch-embedding-size", "100-200-50", "--arch-mlp-bot", "13-16-6",
        "--arch-mlp-top", "30-16-1", "--data-size", "512", "--epochs", "1"]


@pytest.mark.parametrize("extra,words,small", [
    (["--dense-embedding-update"], ["--dense-embedding-update"], SMALL),
    ([], ["6 columns wide", "multiple of 4", "--arch-sparse-feature-size"], D6),
    ([], ["writes columns 6.. of a 30-column Concat", "not 16-byte aligned", "--arch-mlp-bot"], BOT6),
    ([], ["without the q8 extension", "include/ff_hip_q8.h", "--backend"], SMALL),
], ids=["dense-update", "width", "destination", "library"])
def test_compile_refuses_what_the_images_do_not_cover(extra, words, small):
    """Each with the flag to drop, and -- but for the last -- before any library check: the oracle lacks the CTR extension that --eval-batches needs
    as well as this one, and neither is what the refusal names."""
    assert small[small.index("--arch-sparse-feature-size") + 1] in ("8", "6")
    r = _driver("--eval-batches", "2", FLAG, "int8", *extra, small=small)
    assert r.returncode != 0 and "THROUGHPUT" not in r.stdout and "EVAL" not in r.stdout
    for w in words + [FLAG + " int8"]:
        assert w in r.stderr, (w, r.stderr[-2000:])
    assert "CTR extension" not in r.stderr
    if "without the q8 extension" not in words:
        assert "extension" not in r.stderr


def test_sharded_and_replicated_tables_are_refused_in_a_two_rank_job():
    """--row-shard-rows, --column-shard-rows and --replicate-embedding-rows place tables that way only with more than one rank: two driver ranks on the oracle (gloo)."""
    for flag, value, word in (("--column-shard-rows", "150", "is column-sharded"), ("--replicate-embedding-rows", "60", "is replicated"),
                              ("--row-shard-rows", "150", "is row-sharded")):
        r = subprocess.run([sys.executable, LAUNCHER, "-ll:gpu", "2", "--backend", _oracle(), *SMALL, "--eval-batches", "2", FLAG, "int8", flag, value],
                           capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode != 0 and "THROUGHPUT" not in r.stdout
        assert word in r.stderr and flag in r.stderr and FLAG + " int8" in r.stderr, (flag, r.stderr[-2000:])
        assert "extension" not in r.stderr
