"""numpy restatement of include/ffh_bf16.h (bf16 embedding tables): rounding rules and the stochastic-rounding bits."""
import numpy as np

ROUND_STOCHASTIC, ROUND_NEAREST = 0, 1
_U = np.uint64


def mix64(z):
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z + _U(0x9E3779B97F4A7C15)
        z = (z ^ (z >> _U(30))) * _U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _U(27))) * _U(0x94D049BB133111EB)
        return z ^ (z >> _U(31))


def hash64(seed, i):
    with np.errstate(over="ignore"):
        return mix64(mix64(seed) + np.asarray(i, dtype=np.uint64))


def widen(h):
    """bf16 bits (uint16) -> float32, exact."""
    return (np.asarray(h, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def _nan(u):
    return ((u >> np.uint32(16)) | np.uint32(0x40)).astype(np.uint16)


def rne(f):
    u = np.ascontiguousarray(f, dtype=np.float32).view(np.uint32)
    with np.errstate(over="ignore"):
        r = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)
    return np.where((u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000), _nan(u), r)


def sr(f, r):
    u = np.ascontiguousarray(f, dtype=np.float32).view(np.uint32)
    a = u & np.uint32(0x7FFFFFFF)
    with np.errstate(over="ignore"):
        t = ((u + (np.asarray(r, dtype=np.uint32) & np.uint32(0xFFFF))) >> np.uint32(16)).astype(np.uint16)
    t = np.where(a == np.uint32(0x7F800000), (u >> np.uint32(16)).astype(np.uint16), t)
    return np.where(a > np.uint32(0x7F800000), _nan(u), t)


def sr_bits(seed, it, table, rows, cols):
    """16 random bits of (seed, update number, global table, global row, global column); rows / cols broadcast."""
    tkey = hash64(hash64(_U(seed), _U(it)), _U(table))
    rkey = hash64(tkey, np.asarray(rows, dtype=np.uint64))
    cols = np.asarray(cols, dtype=np.uint64)
    with np.errstate(over="ignore"):
        grp = mix64(rkey + (cols >> _U(2)))
    return ((grp >> (_U(16) * (cols & _U(3)))) & _U(0xFFFF)).astype(np.uint32)


def round_table(w32, mode, seed=0, it=0, table=0, col0=0):
    """The bf16 bits the update leaves for the fp32 pre-rounding values w32 [rows][D] of one table."""
    w32 = np.asarray(w32, dtype=np.float32)
    if mode == ROUND_NEAREST:
        return rne(w32)
    R, D = w32.shape
    r = sr_bits(seed, it, table, np.arange(R, dtype=np.uint64)[:, None], (col0 + np.arange(D, dtype=np.uint64))[None, :])
    return sr(w32, r)


def edge_values():
    """+-0, denormals, +-max finite, +-Inf, quiet / signalling NaNs of both signs, halfway cases, as float32."""
    bits = [0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x00008000, 0x00018000, 0x7F7FFFFF, 0xFF7FFFFF,
            0x7F7F8000, 0x7F7F7FFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001,
            0x7FBFFFFF, 0x7F80FFFF, 0xFFFFFFFF, 0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F800001]
    return np.array(bits, dtype=np.uint32).view(np.float32)
