"""CPU tests of the bf16-table extension (include/ff_hip_bf16.h, include/ffh_bf16.h): its symbol list, the library's
exports, the rounding rules restated in numpy against the header compiled on the host, and that a library without the
extension still loads."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import bf16_helpers as B
from dlrm_flexflow_amd import capi

INCLUDE = os.path.join(capi.REPO_ROOT, "include")


def _exported(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_bf16_header_list_declarations_and_prototypes_agree():
    syms = capi.bf16_header_symbols()
    assert len(syms) == len(set(syms)) and syms
    assert set(syms) == set(capi._SIGS_BF16), set(syms) ^ set(capi._SIGS_BF16)
    body = open(capi.BF16_HEADER_PATH).read().split("#define FFH_BF16_API_LIST")[0]
    declared = set(re.findall(r"^\w[\w\s*]*?\b(ffh_[a-z0-9_]+)\s*\(", body, re.M))     # declarations (comments mention helpers)
    assert declared == set(syms), declared ^ set(syms)
    # the base ABI list is untouched by the extension
    assert not set(syms) & set(capi.header_symbols())
    assert set(capi.header_symbols()) == set(capi._SIGS)


def test_hip_library_exports_the_extension():
    from dlrm_flexflow_amd import build
    path = build.build_hip()
    exp = _exported(path)
    missing = [s for s in capi.bf16_header_symbols() if s not in exp]
    assert not missing, missing
    lib = ctypes.CDLL(path)
    lib.ffh_bf16_abi_version.restype = ctypes.c_int
    assert lib.ffh_bf16_abi_version() == capi.bf16_header_abi_version()


def test_ctypes_structs_match_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ff_hip_bf16.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu\\n", sizeof(ffh_emb_table_bf16), offsetof(ffh_emb_table_bf16, table),'
                   ' offsetof(ffh_emb_table_bf16, col0), sizeof(ffh_bf16_rounding), offsetof(ffh_bf16_rounding, counter)); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["cc", "-I", INCLUDE, str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    T, R = capi.EmbTableBf16, capi.Bf16Rounding
    assert got == [ctypes.sizeof(T), T.table.offset, T.col0.offset, ctypes.sizeof(R), R.counter.offset]


@pytest.fixture(scope="module")
def header_lib(tmp_path_factory):
    """include/ffh_bf16.h compiled on the host, behind a throw-away C shim."""
    d = tmp_path_factory.mktemp("bf16h")
    src = d / "shim.c"
    src.write_text('#include "ffh_bf16.h"\n'
                   'void rne_n(const float* f, uint16_t* o, long n){for(long i=0;i<n;i++) o[i]=ffh_bf16_rne(f[i]);}\n'
                   'void sr_n(const float* f, const uint32_t* r, uint16_t* o, long n){for(long i=0;i<n;i++) o[i]=ffh_bf16_sr(f[i], r[i]);}\n'
                   'void bits_n(uint64_t seed, uint64_t it, uint64_t t, const uint64_t* row, const uint64_t* col, uint32_t* o, long n)'
                   '{for(long i=0;i<n;i++) o[i]=ffh_bf16_sr_bits(seed, it, t, row[i], col[i]);}\n'
                   'float widen(uint16_t h){return ffh_bf16_to_f32(h);}\n')
    so = d / "libshim.so"
    subprocess.check_call(["cc", "-O2", "-shared", "-fPIC", "-I", INCLUDE, str(src), "-o", str(so)])
    lib = ctypes.CDLL(str(so))
    P = ctypes.c_void_p
    lib.rne_n.argtypes = [P, P, ctypes.c_long]
    lib.sr_n.argtypes = [P, P, P, ctypes.c_long]
    lib.bits_n.argtypes = [ctypes.c_uint64] * 3 + [P, P, P, ctypes.c_long]
    return lib


def _inputs():
    rng = np.random.default_rng(7)
    u = rng.integers(0, 2**32, 1_000_000, dtype=np.uint64).astype(np.uint32)
    mixed = np.concatenate([u.view(np.float32), rng.standard_normal(100_000).astype(np.float32), B.edge_values()])
    return np.ascontiguousarray(mixed, dtype=np.float32)


def test_nearest_rule_matches_the_header(header_lib):
    f = _inputs()
    out = np.empty(f.size, np.uint16)
    header_lib.rne_n(f.ctypes.data, out.ctypes.data, f.size)
    assert np.array_equal(out, B.rne(f))
    # NaN stays NaN, finite values round to nearest even, +-Inf stay
    e = B.edge_values()
    w = B.widen(B.rne(e))
    assert np.array_equal(np.isnan(w), np.isnan(e))
    assert np.array_equal(np.signbit(w), np.signbit(e))
    assert B.rne(np.float32([1.0 + 2.0**-8]))[0] == 0x3F80          # a halfway case goes to even
    assert B.rne(np.float32([1.0 + 3 * 2.0**-8]))[0] == 0x3F82
    import torch
    fin = np.isfinite(f)
    assert np.array_equal(B.rne(f[fin]), torch.from_numpy(f[fin]).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))


def test_stochastic_rule_matches_the_header(header_lib):
    f = _inputs()
    r = np.random.default_rng(8).integers(0, 2**32, f.size, dtype=np.uint64).astype(np.uint32)
    out = np.empty(f.size, np.uint16)
    header_lib.sr_n(f.ctypes.data, r.ctypes.data, out.ctypes.data, f.size)
    assert np.array_equal(out, B.sr(f, r))
    e = B.edge_values()
    w = B.widen(B.sr(e, np.full(e.size, 0xFFFF, np.uint32)))
    assert np.array_equal(np.isnan(w), np.isnan(e))                  # a NaN never becomes an Inf, an Inf never a NaN
    assert np.array_equal(np.isinf(w) & ~np.isinf(e), (np.abs(e) > 3.389e38) & ~np.isinf(e) & ~np.isnan(e))


def test_stochastic_bits_match_the_header(header_lib):
    rng = np.random.default_rng(9)
    n = 200_000
    row = rng.integers(0, 2**40, n, dtype=np.uint64)
    col = rng.integers(0, 4096, n, dtype=np.uint64)
    for seed, it, t in [(0, 0, 0), (1234, 7, 25), (2**63 + 5, 2**40, 63)]:
        out = np.empty(n, np.uint32)
        header_lib.bits_n(seed, it, t, row.ctypes.data, col.ctypes.data, out.ctypes.data, n)
        assert np.array_equal(out, B.sr_bits(seed, it, t, row, col))
    # roughly uniform 16-bit draws, and a different update number gives different bits
    a = B.sr_bits(5, 0, 1, row, col)
    b = B.sr_bits(5, 1, 1, row, col)
    assert abs(a.mean() / 65535.0 - 0.5) < 0.01 and (a != b).mean() > 0.99


def test_library_without_the_extension_still_loads(oracle):
    """The CPU oracle exports the base ABI only: it loads as before, and asking it for the extension is a clear error."""
    be = oracle.lib()
    assert be.backend == "oracle-cpu"
    with pytest.raises(capi.FFHError, match="bf16-table extension"):
        capi.bf16_api(be)


def test_host_backend_loads_the_oracle_without_the_extension():
    """host/backend loads the extension optionally: the driver on the oracle (no extension) runs as before."""
    import dlrm_helpers as H
    exe = os.path.join(capi.REPO_ROOT, "dlrm_flexflow_amd", "host", "dlrm")
    args = [exe, "--backend", H.oracle_backend(), "-ll:gpu", "1", "-b", "32", "--arch-sparse-feature-size", "8",
            "--arch-embedding-size", "100-100", "--arch-mlp-bot", "13-8", "--arch-mlp-top", "24-1", "--epochs", "1", "--data-size", "64"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "THROUGHPUT = " in r.stdout
