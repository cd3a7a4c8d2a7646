"""GPU tests of the DCNv2 low-rank cross interaction (include/ff_hip_cross.h): the two entries through the C-ABI against
ffmodel.cross_reference bit for bit, and the whole model (--arch-interaction-op dcn) against a live torch float64 model
(tests/cross_helpers.py) -- eager and traced, SGD and Adam, the math modes, the kernel routes, --deterministic, the gradient fan-in of x_0 and
two ranks sharing the GPU.

Bitwise comparison: ffmodel.cross_reference is float32 numpy, two separately rounded operations per element like the kernels, so every
number that is not a NaN must agree in all 32 bits (signed zeros, subnormals and infinities included).  Where the arithmetic makes a NaN
(0 * inf, inf - inf) the POSITIONS must agree; the payload is not compared: IEEE 754 leaves the sign and payload of a generated NaN to the
implementation, and x86 (0xFFC00000) and the GPU (0x7FC00000) choose differently."""
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
from dlrm_flexflow_amd import capi, ffmodel
import cross_helpers as X

pytestmark = pytest.mark.gpu

HIP = capi.HIP_LIB_PATH
SENTINEL = np.float32(-7.25e9)
SHAPES = [(1, 1), (3, 5), (7, 64), (64, 67), (129, 128), (300, 3456)]
MODES = [capi.CROSS_SKIP, capi.CROSS_STORE, capi.CROSS_ADD]
SPECIALS = np.array([0.0, -0.0, 1e-40, -3e-42, np.inf, -np.inf, 1.17549435e-38, 3.0e38], np.float32)


@pytest.fixture(scope="module")
def cross(hip):
    """Every test goes through here first: a library without the extension fails the test plainly (capi.FFHError), before any driver starts."""
    return capi.cross_api(hip)


class Buf:
    """A [batch][dim] operand inside a sentinel-filled allocation: `off` floats in front, row stride ld, two rows behind the batch."""

    def __init__(self, batch, dim, ld, off, values):
        self.batch, self.dim, self.ld, self.off = batch, dim, ld, off
        self.host = np.full(off + (batch + 2) * ld + 4, SENTINEL, np.float32)
        self.view(self.host)[:] = values
        self.dev = torch.from_numpy(self.host).to("cuda:0")
        self.ptr = self.dev.data_ptr() + 4 * off

    def view(self, flat):
        return np.lib.stride_tricks.as_strided(flat[self.off:], (self.batch, self.dim), (4 * self.ld, 4))

    def expect(self, values=None):
        """the whole allocation as it must look afterwards: untouched, or with the [batch][dim] elements replaced"""
        e = self.host.copy()
        if values is not None:
            self.view(e)[:] = values
        return e

    def got(self):
        return self.dev.cpu().numpy()


def same_bits(got, exp, what):
    got, exp = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(exp, np.float32)
    assert got.shape == exp.shape, what
    gn, en = np.isnan(got), np.isnan(exp)
    assert np.array_equal(gn, en), f"{what}: NaN positions differ at {np.argwhere(gn != en)[:5].tolist()}"
    bad = (got.view(np.uint32) != exp.view(np.uint32)) & ~en
    assert not bad.any(), f"{what}: {int(bad.sum())} elements differ, first {np.argwhere(bad)[:5].tolist()}: {got[bad][:5]} vs {exp[bad][:5]}"


def values(batch, dim, seed):
    """random values with every special (signed zeros, subnormals, infinities, the smallest normal, a huge one) sprinkled in, at positions that
    make the products and sums of the operands meet: inf * 0, inf - inf, subnormal results, overflow"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-2, 2, (batch, dim)).astype(np.float32)
    flat = a.reshape(-1)
    n = flat.size
    pos = rng.permutation(n)[:max(1, n // 5)]
    flat[pos] = SPECIALS[rng.integers(0, len(SPECIALS), pos.size)]
    return a


def layout(dim, padded):
    """(ld, offset of operand k): tight, or ld = dim rounded up to 32 with ONE operand (the second) based 4 bytes off -- the scalar path"""
    if not padded:
        return dim, lambda k: 0
    return (dim + 31) // 32 * 32, lambda k: 1 if k == 1 else 0


# ---- 1. the entries against cross_reference, bit for bit -------------------------------------------------------------------------------
@pytest.mark.parametrize("padded", [False, True], ids=["tight", "padded"])
@pytest.mark.parametrize("aliased", [False, True], ids=["x0_xl", "xl_is_x0"])
@pytest.mark.parametrize("batch,dim", SHAPES)
def test_cross_fwd_equals_the_reference_bit_for_bit(cross, batch, dim, padded, aliased):
    ld, off = layout(dim, padded)
    x0 = Buf(batch, dim, ld, off(0), values(batch, dim, 1))
    v = Buf(batch, dim, ld, off(1), values(batch, dim, 2))
    xl = x0 if aliased else Buf(batch, dim, ld, off(2), values(batch, dim, 3))
    y = Buf(batch, dim, ld, off(3), SENTINEL)
    cross.call("ffh_cross_fwd", y.ptr, ld, x0.ptr, ld, v.ptr, ld, xl.ptr, ld, batch, dim, None)
    torch.cuda.synchronize()
    exp = ffmodel.cross_reference(x0.view(x0.host), v.view(v.host), xl.view(xl.host))
    same_bits(y.got(), y.expect(exp), "y (pad columns and the rows behind the batch included)")
    for name, b in (("x0", x0), ("v", v), ("xl", xl)):
        assert b.got().tobytes() == b.host.tobytes(), f"{name} was written"


def run_bwd(cross, batch, dim, padded, mode_x0, mode_xl, aliased):
    ld, off = layout(dim, padded)
    dy = Buf(batch, dim, ld, off(0), values(batch, dim, 4))
    x0 = Buf(batch, dim, ld, off(1), values(batch, dim, 5))
    v = Buf(batch, dim, ld, off(2), values(batch, dim, 6))
    dv = Buf(batch, dim, ld, off(3), SENTINEL)
    dx0 = Buf(batch, dim, ld, off(4), values(batch, dim, 7))          # what an ADD adds to
    dxl = dx0 if aliased else Buf(batch, dim, ld, off(5), values(batch, dim, 8))
    rc = cross.rc("ffh_cross_bwd", dy.ptr, ld, x0.ptr, ld, v.ptr, ld, dv.ptr, ld, dx0.ptr, ld, mode_x0, dxl.ptr, ld, mode_xl, batch, dim, None)
    torch.cuda.synchronize()
    return rc, dy, x0, v, dv, dx0, dxl


def check_bwd(rc, dy, x0, v, dv, dx0, dxl, mode_x0, mode_xl, aliased):
    assert rc == capi.FFH_OK
    g_dv, g0, gl = ffmodel.cross_reference_backward(dy.view(dy.host), x0.view(x0.host), v.view(v.host), aliased=aliased)
    same_bits(dv.got(), dv.expect(g_dv), "dv")

    def after(buf, mode, g):
        if mode == capi.CROSS_SKIP:
            return buf.expect()
        with np.errstate(all="ignore"):
            return buf.expect(g if mode == capi.CROSS_STORE else buf.view(buf.host) + g)
    same_bits(dx0.got(), after(dx0, mode_x0, g0), "dx0")
    if not aliased:
        same_bits(dxl.got(), after(dxl, mode_xl, gl), "dxl")
    for name, b in (("dy", dy), ("x0", x0), ("v", v)):
        assert b.got().tobytes() == b.host.tobytes(), f"{name} was written"


@pytest.mark.parametrize("padded", [False, True], ids=["tight", "padded"])
@pytest.mark.parametrize("batch,dim", SHAPES)
def test_cross_bwd_equals_the_reference_bit_for_bit(cross, batch, dim, padded):
    """every shape in the two forms the model issues: ADD / ADD on separate buffers, and layer 0's one accumulated write"""
    for aliased in (False, True):
        out = run_bwd(cross, batch, dim, padded, capi.CROSS_ADD, capi.CROSS_ADD, aliased)
        check_bwd(*out, capi.CROSS_ADD, capi.CROSS_ADD, aliased)


@pytest.mark.parametrize("mode_xl", MODES)
@pytest.mark.parametrize("mode_x0", MODES)
@pytest.mark.parametrize("batch,dim,padded", [(64, 67, False), (129, 128, False), (129, 128, True)], ids=["scalar", "vector", "vector-shape-off-base"])
def test_cross_bwd_all_nine_mode_combinations(cross, batch, dim, padded, mode_x0, mode_xl):
    out = run_bwd(cross, batch, dim, padded, mode_x0, mode_xl, False)
    check_bwd(*out, mode_x0, mode_xl, False)


@pytest.mark.parametrize("mode", [capi.CROSS_STORE, capi.CROSS_ADD])
@pytest.mark.parametrize("batch,dim", [(64, 67), (129, 128)])
def test_cross_bwd_one_buffer_for_dx0_and_dxl(cross, batch, dim, mode):
    out = run_bwd(cross, batch, dim, False, mode, mode, True)
    check_bwd(*out, mode, mode, True)


@pytest.mark.parametrize("mode_x0,mode_xl", [(capi.CROSS_STORE, capi.CROSS_ADD), (capi.CROSS_ADD, capi.CROSS_STORE), (capi.CROSS_ADD, capi.CROSS_SKIP),
                                             (capi.CROSS_SKIP, capi.CROSS_STORE)])
def test_cross_bwd_one_buffer_with_mismatched_modes_is_a_bad_argument(cross, mode_x0, mode_xl):
    rc, dy, x0, v, dv, dx0, dxl = run_bwd(cross, 7, 64, False, mode_x0, mode_xl, True)
    assert rc == capi.FFH_ERR_BAD_ARG
    for b in (dv, dx0):
        assert b.got().tobytes() == b.host.tobytes()          # nothing was launched


def test_bad_arguments_are_refused(cross):
    b = Buf(3, 5, 8, 0, 1.0)
    assert cross.rc("ffh_cross_fwd", b.ptr, 4, b.ptr, 8, b.ptr, 8, b.ptr, 8, 3, 5, None) == capi.FFH_ERR_BAD_ARG          # ld < dim
    assert cross.rc("ffh_cross_fwd", b.ptr, 8, None, 8, b.ptr, 8, b.ptr, 8, 3, 5, None) == capi.FFH_ERR_BAD_ARG          # null input
    assert cross.rc("ffh_cross_bwd", b.ptr, 8, b.ptr, 8, b.ptr, 8, b.ptr, 8, None, 8, 3, None, 8, 0, 3, 5, None) == capi.FFH_ERR_BAD_ARG   # unknown mode
    assert cross.rc("ffh_cross_fwd", b.ptr, 8, b.ptr, 8, b.ptr, 8, b.ptr, 8, 0, 5, None) == capi.FFH_OK                   # batch 0: nothing to do


# ---- 2. the whole model against live torch float64 ----------------------------------------------------------------------------------------
_REF = {}


def model_run(L, R, optimizer="sgd", trace=False, extra=()):
    """(got, exp, aux): the torch side depends on (L, R, optimizer) only (seeded initial state, one resident batch): computed once, shared"""
    key = (L, R, optimizer)
    got, exp, aux = X.run_dcn(HIP, L, R, steps=3, trace=trace, optimizer=optimizer, extra=extra, want_torch=key not in _REF)
    if key not in _REF:
        _REF[key] = (exp, aux[1])
    return got, _REF[key][0], (aux[0], _REF[key][1])


@pytest.mark.parametrize("trace", [False, True], ids=["eager", "traced"])
@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
@pytest.mark.parametrize("R", [8, 32])
@pytest.mark.parametrize("L", [1, 3])
def test_dcn_model_equals_torch_float64(cross, L, R, optimizer, trace):
    got, exp, _ = model_run(L, R, optimizer, trace)
    X.assert_close(got, exp, f"L={L} R={R} {optimizer}")


def test_dcn_model_in_the_split_mode_holds_the_fp32_bound(cross):
    got, exp, _ = model_run(3, 32, extra=["--fp32-split-bf16x3"])
    X.assert_close(got, exp, "--fp32-split-bf16x3")


def test_dcn_model_in_tensor_op_mode(cross):
    """tests/test_bf16_mode.py bounds a whole step in this mode in one way that does not need a second kernel library: the prediction of a
    tensor-op run stays within 2e-2 of the fp32 run (test_driver_flag_reaches_the_kernels_cpu).  The same bound here, against torch; every
    parameter finite.  (At these widths -- 144, 64, 32 -- no layer reaches the bf16 pipe's minimum, so the run is in fact the fp32 one.)"""
    got, exp, _ = model_run(3, 32, extra=["--allow-tensor-op-math-conversion"])
    for k, v in got.items():
        assert np.isfinite(v).all(), k
    assert np.abs(got["pred"].astype(np.float64) - exp["pred"]).max() < 2e-2


@pytest.mark.parametrize("flag", ["--no-mlp-chain", "--no-fused-pair", "--no-dx-colsum"])
def test_dcn_model_is_independent_of_the_kernel_route(cross, flag):
    got, exp, _ = model_run(3, 8, extra=[flag])
    X.assert_close(got, exp, flag)
    base, _, _ = model_run(3, 8)
    X.assert_close(got, base, flag + " against the default routes")


def test_dcn_model_deterministic_runs_are_bit_identical(cross):
    a, exp, _ = model_run(3, 8, extra=["--deterministic"])
    b, _, _ = model_run(3, 8, extra=["--deterministic"])
    X.assert_close(a, exp, "--deterministic")
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_gradient_reaching_the_concat_sums_all_four_consumers(cross):
    """L = 3: x_0 feeds V_0 and the three combines (layer 0's twice).  A consumer that stored where it must add would drop the others.  (The
    bottom MLP's slice of the buffer is read behind the ReLU mask its last layer applies in place: tests/cross_helpers.py.)"""
    _, _, (got, exp) = model_run(3, 8)
    assert got.shape == exp.shape == (X.B, X.WIDTH)
    np.testing.assert_allclose(got.astype(np.float64), exp, rtol=X.RTOL, atol=X.ATOL)
    assert np.abs(exp).max() > 100 * X.ATOL          # the comparison is not between zeros


def test_two_ranks_sharing_the_gpu_equal_one_rank(cross, tmp_path):
    L, R = 3, 8
    worker = os.path.join(ROOT, "tests", "_dist_worker_cross.py")
    port = str(29900 + os.getpid() % 90)
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
        procs.append(subprocess.Popen(["python", worker, str(tmp_path), str(L), str(R)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=600)[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    z = [np.load(os.path.join(tmp_path, f"rank{r}.npz")) for r in range(2)]
    one, _, _ = X.run_dcn(HIP, L, R, steps=2, want_torch=False)
    seen = set()
    for r in range(2):
        assert int(z[r]["allreduce_calls"]) >= 2          # the cross layers' gradients travelled with the MLPs'
        np.testing.assert_allclose(z[r]["pred"], one["pred"][r * X.B // 2:(r + 1) * X.B // 2], rtol=X.RTOL, atol=X.ATOL, err_msg=f"pred rank {r}")
        for k in z[r].files:
            if "/" not in k:
                continue
            np.testing.assert_allclose(z[r][k], one[k], rtol=X.RTOL, atol=X.ATOL, err_msg=f"{k} rank {r}")
            seen.add(k)
    assert seen == set(one) - {"pred"}, set(one) - seen          # every parameter is held by some rank
