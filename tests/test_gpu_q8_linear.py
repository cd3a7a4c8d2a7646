"""GPU tests (-m gpu) of the int8 Linear kernels (include/ffh_q8_linear.h, csrc/linear_q8.hip) through capi.q8_linear_api: both quantizers and the
GEMM against the numpy restatement of the rule (ffmodel.q8_linear_quantize_reference / q8_linear_reference), bit for bit -- the int32 sums are exact
and the three fp32 operations are specified, so nothing here is a tolerance except the sigmoid's own rounding (tests/linear_helpers.py: 8 eps)."""
import numpy as np
import pytest
import torch

from dlrm_flexflow_amd import capi, ffmodel
from chain_helpers import EPS32

pytestmark = pytest.mark.gpu
NONE, RELU, SIG = capi.AC_MODE_NONE, capi.AC_MODE_RELU, capi.AC_MODE_SIGMOID
GUARD = 64              # elements behind every buffer that no call may touch
MARK8, MARKF = 0x5A, -777.25


@pytest.fixture(scope="module")
def q8l(hip):
    return capi.q8_linear_api(hip)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _strided(v, ld):
    """[rows][ld] device buffer with v in its first columns and NaN behind them"""
    buf = np.full((v.shape[0], ld), np.nan, np.float32)
    buf[:, :v.shape[1]] = v
    return _dev(buf)


def _image(q8l, rows, width):
    ldq = q8l.ldq(width)
    assert ldq == (width + 63) // 64 * 64
    return (torch.full((rows * ldq + GUARD,), MARK8, dtype=torch.int8, device="cuda"), torch.full((rows + GUARD,), MARKF, device="cuda"), ldq)


def _check_image(codes, scales, ldq, v, what):
    """codes and scales equal the rule, the K padding is zero, the guards are untouched"""
    rows, width = v.shape
    q, s = ffmodel.q8_linear_quantize_reference(v)
    got = codes.cpu().numpy()
    img = got[:rows * ldq].reshape(rows, ldq)
    assert np.array_equal(img[:, :width], q), what
    assert not img[:, width:].any() and np.all(got[rows * ldq:] == MARK8), what
    gs = scales.cpu().numpy()
    assert np.array_equal(gs[:rows].view(np.uint32), s.view(np.uint32)) and np.all(gs[rows:] == np.float32(MARKF)), what


def _rows(rng, rows, width):
    v = rng.standard_normal((rows, width)).astype(np.float32)
    v[0] = 0.0                                                       # scale 0, codes 0
    v[1, 3] = -9.0                                                   # the extreme is negative
    v[2] = (np.arange(width) % 120 + 0.5) * np.where(np.arange(width) % 2, -1.0, 1.0)      # inv = 1: every value lands on .5
    v[2, 0] = 127.0
    return v


@pytest.mark.parametrize("width,rows", [(64, 70), (130, 37), (1040, 9), (1040, 2048 * 4 + 5)], ids=["64", "130", "1040", "1040-past-the-cap"])
def test_quantizers_equal_the_numpy_rule(q8l, width, rows):
    assert q8l.quantize_max_workgroups() == 2048
    v = _rows(np.random.default_rng(width + rows), rows, width)
    ld = width + 3
    src = _strided(v, ld)
    codes, scales, ldq = _image(q8l, rows, width)
    q8l.quantize_rows(src, ld, codes, scales, rows, width)
    _check_image(codes, scales, ldq, v, "rows")
    # the weights' entry: the same matrix as a list of two (and a third of another width), one launch
    cut, w2 = 5, 64
    v2 = _rows(np.random.default_rng(1), 6, w2)
    (ca, sa, _), (cb, sb, _), (cc, sc, ldq2) = _image(q8l, cut, width), _image(q8l, rows - cut, width), _image(q8l, 6, w2)
    q8l.quantize_weights([(src, ld, ca, sa, cut, width), (_dev(v2), w2, cc, sc, 6, w2), (src[cut:], ld, cb, sb, rows - cut, width)])
    _check_image(ca, sa, ldq, v[:cut], "weights, first matrix")
    _check_image(cc, sc, ldq2, v2, "weights, second matrix")
    _check_image(cb, sb, ldq, v[cut:], "weights, third matrix")


def _operands(rng, batch, n_in, n_out, extreme):
    if extreme:      # codes of +-127 throughout: |acc| reaches 127^2 in
        x = np.where(rng.random((batch, n_in)) < 0.02, -1.5, 1.5).astype(np.float32)
        W = np.where(rng.random((n_out, n_in)) < 0.02, -0.25, 0.25).astype(np.float32)
        x[0], W[0] = 1.5, 0.25
    else:
        x, W = rng.standard_normal((batch, n_in)).astype(np.float32), (rng.standard_normal((n_out, n_in)) * 0.1).astype(np.float32)
    return x, W, rng.standard_normal(n_out).astype(np.float32)


# the four shapes of the 64 x 64 tiles; 128 x 128 tiles from 256 of them on (16 x 16, both edges partial, three K steps); +-127 throughout at in = 1040
# (the largest sum there is 127^2 1040 = 16774160, just below 2^24) and at in = 1041 (16790289: odd and past 2^24, so (float)acc rounds)
@pytest.mark.parametrize("batch,n_in,n_out,extreme", [(1, 64, 64, False), (33, 130, 200, False), (129, 1040, 257, False), (300, 64, 513, False),
                                                      (1925, 130, 2047, False), (70, 1040, 66, True), (70, 1041, 66, True)],
                         ids=lambda v: str(int(v)))
def test_gemm_equals_the_numpy_rule(q8l, batch, n_in, n_out, extreme):
    x, W, bias = _operands(np.random.default_rng(batch + n_in), batch, n_in, n_out, extreme)
    (xq, sx, ldq), (wq, sw, _) = _image(q8l, batch, n_in), _image(q8l, n_out, n_in)
    q8l.quantize_rows(_dev(x), n_in, xq, sx, batch, n_in)
    q8l.quantize_weights([(_dev(W), n_in, wq, sw, n_out, n_in)])
    _check_image(xq, sx, ldq, x, "x")
    if extreme:
        acc = np.abs(ffmodel.q8_linear_quantize_reference(x)[0].astype(np.int64) @ ffmodel.q8_linear_quantize_reference(W)[0].astype(np.int64).T)
        assert acc.max() == 127 * 127 * n_in and (acc.max() > 2 ** 24) == (n_in > 1040) and np.any(acc % 2 == 1) == (n_in > 1040)
    dbias = _dev(bias)
    for with_bias in (True, False):
        for act in (NONE, RELU, SIG):
            # (the sigmoid: the exact pre-activation through a float64 sigmoid, within the rounding of expf and the division)
            want = ffmodel.q8_linear_reference(x, W, bias if with_bias else None, act, pre_activation=act == SIG)
            ref = 1.0 / (1.0 + np.exp(-want.astype(np.float64)))
            for ldy in (n_out, (n_out + 3) // 4 * 4 + 4, n_out + 1):     # as wide as the output; 16-byte rows with a gap; dword stores
                y = torch.full((batch * ldy + GUARD,), MARKF, device="cuda")
                q8l.fwd(xq, wq, sx, sw, dbias if with_bias else None, y, ldy, batch, n_in, n_out, act)
                got = y.cpu().numpy()
                rows = got[:batch * ldy].reshape(batch, ldy)
                what = (with_bias, ldy, act)
                assert np.all(rows[:, n_out:] == np.float32(MARKF)) and np.all(got[batch * ldy:] == np.float32(MARKF)), what
                if act == SIG:
                    assert np.all(np.abs(rows[:, :n_out] - ref) <= 8 * EPS32 * np.abs(ref)), what
                else:
                    assert np.array_equal(rows[:, :n_out].view(np.uint32), want.view(np.uint32)), what
    assert np.all(xq.cpu().numpy()[batch * ldq:] == MARK8) and np.all(wq.cpu().numpy()[n_out * ldq:] == MARK8)


def test_bad_arguments_are_refused_and_write_nothing(q8l):
    batch, n_in, n_out = 8, 64, 64
    (xq, sx, _), (wq, sw, _) = _image(q8l, batch, n_in), _image(q8l, n_out, n_in)
    x, y = torch.ones(batch, n_in, device="cuda"), torch.full((batch * n_out,), MARKF, device="cuda")
    bad = capi.FFH_ERR_BAD_ARG
    assert q8l.fwd_rc(None, wq, sx, sw, None, y, n_out, batch, n_in, n_out, NONE) == bad
    assert q8l.fwd_rc(xq, wq, sx, sw, None, None, n_out, batch, n_in, n_out, NONE) == bad
    assert q8l.fwd_rc(xq, wq, sx, sw, None, y, n_out, -1, n_in, n_out, NONE) == bad
    assert q8l.fwd_rc(xq, wq, sx, sw, None, y, n_out - 1, batch, n_in, n_out, NONE) == bad
    assert q8l.quantize_rows_rc(None, n_in, xq, sx, batch, n_in) == bad and q8l.quantize_rows_rc(x, n_in, xq, None, batch, n_in) == bad
    assert q8l.quantize_rows_rc(x, n_in, xq, sx, -1, n_in) == bad and q8l.quantize_rows_rc(x, n_in - 1, xq, sx, batch, n_in) == bad
    assert q8l.quantize_weights_rc(None) == bad and q8l.quantize_weights_rc([]) == bad
    assert q8l.quantize_weights_rc([(x, n_in, None, sw, batch, n_in)]) == bad
    torch.cuda.synchronize()
    assert torch.all(y == MARKF) and torch.all(xq == MARK8) and torch.all(wq == MARK8) and torch.all(sx == MARKF) and torch.all(sw == MARKF)
