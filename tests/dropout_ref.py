"""The dropout stream from its definition, and the table of cases the CPU and GPU stream tests share.

A dropout decision is a pure function of (seed, epoch, stream index j, thr16) (csrc/common.h, "dropout decisions"):

    keep(j)  <=>  U16(j) >= thr16

U16(j) is a 16-bit uniform.  For i = 1 .. 16, bit 16 - i of U16(j) is bit j & 31 of output word (j >> 5) & 3 of

    Philox4x32-10(counter = {lo32(j >> 7), hi32(j >> 7), epoch, i}, key = {lo32 seed, hi32 seed})

The kernels never form U16: they walk the bit planes with an and/or recurrence and skip the planes below the lowest set bit
of thr16.  This file does the opposite on purpose: u16() materialises the number and keep() compares it, with no plane
skipped and no recurrence, so a slip in the kernels' walk (a plane too few, and/or swapped, a counter word dropped) cannot
also be made here.  philox4x32_10 is held to the Random123 known answers by test_dropout_stream_cpu.py, which ties the
whole chain to something outside the project.  (Philox is evaluated once per block j >> 7 and bit plane, not once per
element: the 128 elements of a block share the call by definition, so that is a cache, not the kernels' structure.)

Decoding the dense first-layer products (dense_operands / decode_fwd / decode_bwd).  X[r, k] = 2^(k // 128), W[k, k % 128]
= 1, every other W zero, so with N[r, c] = sum_q 2^q keep(r K + 128 q + c)

    out[r, c] = sum_k X~[r, k] W[k, c] = scale . N[r, c],        q < ceil(K / 128) <= 12:  N < 4096

and dout[r, r % 128] = 2^(r // 128) gives dW[k, c] = scale . 2^(k // 128) . sum_q 2^q keep((128 q + c) K + k), q <= 1.
Every operand is a power of two up to 2^11: exact in f32 and in bf16, so the bf16x3 kernels' first plane holds X whole.
The scale 1 / (1 - p) is not a power of two, so a kernel that multiplies X by it (or folds it into W, or splits it into
three bf16 planes) rounds each term and the sum: out = scale . N . (1 + d).  Every term is >= 0, so sum |terms| is the value
itself and the dispatch tests' own bound gives |d| <= 9 eps_f32 (test_spmm_dispatch_gpu.py: 8, 9 where the scale is folded
into W).  N < 4096, so |out / scale - N| < 4096 . 9 . 2^-23 < 0.005: rint(out / scale) is N exactly, and bit q of N is the
decision.  The decode also REQUIRES |out / scale - N| <= 2^-6, so a product that is off by more fails instead of being
rounded into place.  The sparse products are decoded the same way (sparse_*: N < 256).
"""
import numpy as np

M32 = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------------------ Philox
def philox4x32_10(ctr, key):
    """Philox4x32 with 10 rounds (Salmon et al., SC'11).  ctr: four words, key: two words; each a Python int or an integer
    array (broadcast together).  -> uint64 array [..., 4] of 32-bit words"""
    c = [np.asarray(x, np.uint64) & np.uint64(M32) for x in ctr]
    k = [int(x) & M32 for x in key]
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]                      # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(0xCD9E8D57) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(M32)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(M32)
        c = [hi1 ^ c[1] ^ np.uint64(k[0]), lo1, hi0 ^ c[3] ^ np.uint64(k[1]), lo0]
        k = [(k[0] + 0x9E3779B9) & M32, (k[1] + 0xBB67AE85) & M32]
    return np.stack(np.broadcast_arrays(*c), axis=-1)


# Random123's kat_vectors for philox4x32, 10 rounds: (counter, key, output)
KNOWN_ANSWERS = (
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff), (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


# ------------------------------------------------------------------------------------------------------ the definition
def u16(seed, epoch, j):
    """the materialised 16-bit uniform of stream indices j (any shape, values below 2^64) -> int64 array"""
    j = np.asarray(j, np.uint64)
    blocks, inv = np.unique(j >> np.uint64(7), return_inverse=True)
    inv = inv.reshape(j.shape)
    word = ((j >> np.uint64(5)) & np.uint64(3)).astype(np.int64)
    bit = j & np.uint64(31)
    u = np.zeros(j.shape, np.int64)
    for i in range(1, 17):
        out = philox4x32_10((blocks & np.uint64(M32), blocks >> np.uint64(32), int(epoch), i), (int(seed) & M32, (int(seed) >> 32) & M32))
        plane = ((out[inv, word] >> bit) & np.uint64(1)).astype(np.int64)
        u |= plane << (16 - i)
    return u


def u16_range(seed, epoch, start, n):
    """u16 of the n consecutive indices from start"""
    return u16(seed, epoch, np.arange(n, dtype=np.uint64) + np.uint64(start))


def keep(seed, epoch, j, thr16):
    return u16(seed, epoch, j) >= int(thr16)


def thr16(p):
    """dropout_threshold (csrc/common.h), in float32 as the host computes it"""
    t = int(np.float32(p) * np.float32(65536.0) + np.float32(0.5))
    return min(65535, max(0, t))


def scale(p):
    """the host's 1 / (1 - p) on floats"""
    return np.float32(1) / (np.float32(1) - np.float32(p))


def p_of(t):
    """a rate whose threshold is t: t / 65536 is exact in float32, and t + 0.5 truncates to t"""
    p = t / 65536.0
    assert float(np.float32(p)) == p and thr16(p) == t
    return p


# ------------------------------------------------------------------------------------------------------------ the table
P_EDGE = float(np.float32(2.0 ** -17))                         # p * 65536 + 0.5 == 1.0 exactly
P_BELOW, P_ABOVE = (float(np.nextafter(np.float32(P_EDGE), np.float32(s))) for s in (0, 1))   # the floats either side
# The float below 2^-17 does NOT give 0: p * 65536 + 0.5 = 1 - 2^-25 lies midway between two floats and rounds to the even
# one, 1.0.  The threshold really turns from 0 to 1 one float further down, between P_ZERO and P_BELOW.
P_ZERO = float(np.nextafter(np.float32(P_BELOW), np.float32(0)))
RATES = (("p0.1", 0.1), ("p0.25", 0.25), ("p0.3", 0.3), ("p0.9", 0.9), ("p2^-17-2ulp", P_ZERO), ("p2^-17-1ulp", P_BELOW),
         ("p2^-17+1ulp", P_ABOVE), ("p0.999999", 0.999999))     # entry points take these as they are
THR_RAW = (0, 1, 2, 0x4000, 0x8000, 0xC000, 0x5555, 0xFFFE, 0xFFFF)
# (label, thr16, p): the raw thresholds through p_of, the rates as given
THR = tuple((f"thr{t:#06x}", t, p_of(t)) for t in THR_RAW) + tuple((label, thr16(p), p) for label, p in RATES)
OFFSETS = (0, 1, 31, 33, 77, 96, 127, 128, 640, 2 ** 32 - 50, 2 ** 32 + 96, 2 ** 39 - 200, 2 ** 45 + 77)
SEEDS = ((42, 5), (0xabcdef12345, 0xFFFFFFFF), (2 ** 64 - 1, 0))


def n_planes(t):
    """bit planes the kernels read for threshold t (none at 0)"""
    return 0 if t == 0 else 16 - ((t & -t).bit_length() - 1)


_U16 = {}


def u16_cached(seed, epoch, start, n):
    """u16_range, computed once per (seed, epoch, start) and shared by every threshold and test (read-only)"""
    key = (seed, epoch, start)
    if key not in _U16 or _U16[key].size < n:
        a = u16_range(seed, epoch, start, n)
        a.setflags(write=False)
        _U16[key] = a
    return _U16[key][:n]


def keep_range(seed, epoch, start, n, t):
    return u16_cached(seed, epoch, start, n) >= int(t)


# ---------------------------------------------------------------------------------- decoding the first-layer products
DECODE_TOL = 2.0 ** -6


def _exact_int(q, what):
    n = np.rint(q)
    err = float(np.abs(q - n).max()) if q.size else 0.0
    assert err <= DECODE_TOL, f"{what}: a product is {err:.3e} from a whole multiple of the scale"
    return n.astype(np.int64)


def dense_operands(m, K):
    """-> X [m, K], W [K, 128], dout [m, 128] of the module docstring"""
    X = np.broadcast_to(np.exp2(np.arange(K) // 128).astype(np.float32), (m, K)).copy()
    W = np.zeros((K, 128), np.float32)
    W[np.arange(K), np.arange(K) % 128] = 1
    dout = np.zeros((m, 128), np.float32)
    dout[np.arange(m), np.arange(m) % 128] = np.exp2(np.arange(m) // 128)
    return X, W, dout


def decode_fwd(out, K, sc):
    """out [m, 128] of the forward on dense_operands -> keep [m, K]"""
    N = _exact_int(np.asarray(out, np.float64) / float(sc), "forward")
    assert not N[:, K:].any(), "a column that no X column feeds is not zero"
    k = np.arange(K)
    return ((N[:, k % 128] >> (k // 128)) & 1).astype(bool)


def decode_bwd(dw, m, sc):
    """dW [K, 128] of the weight gradient on dense_operands -> keep [m, K]"""
    K = dw.shape[0]
    N = _exact_int(np.asarray(dw, np.float64) / (float(sc) * np.exp2(np.arange(K) // 128)[:, None]), "weight gradient")
    r = np.arange(m)
    assert int(N.max(initial=0)) < 1 << ((m + 127) // 128)
    return ((N[:, r % 128].T >> (r // 128)[:, None]) & 1).astype(bool)


def sparse_fwd_operands(fp, p):
    """the t-th stored value of a row is 2^t (rows of at most 8 values), W is all ones: out[r, c] = scale . sum_t 2^t keep"""
    fp = np.asarray(fp, np.int64)
    t = np.arange(fp[-1]) - np.repeat(fp[:-1], np.diff(fp))
    assert t.max() < 8
    return np.exp2(t).astype(np.float32), t


def decode_sparse_fwd(out, fp, t, sc):
    """-> keep [nnz]; every column of out carries the same sum"""
    N = _exact_int(np.asarray(out, np.float64) / float(sc), "sparse forward")
    assert np.all(N == N[:, :1]), "columns of a row differ"
    rows = np.repeat(np.arange(np.asarray(fp).size - 1), np.diff(fp))
    return ((N[rows, 0] >> t) & 1).astype(bool)


SPARSE_BWD_ROWS = 8                                            # rows (bits) per output column and call


def sparse_bwd_douts(n, p):
    """stored values all 1; call s covers rows [s B, (s + 1) B), B = 8 p: dout[r, i % p] = 2^(i // p), i = r - s B.  Two entries
    of one column of X lie in different rows, so they land in different (output column, bit) places of dW."""
    B = SPARSE_BWD_ROWS * p
    for s in range(-(-n // B)):
        r = np.arange(s * B, min(n, (s + 1) * B))
        d = np.zeros((n, p), np.float32)
        d[r, (r - s * B) % p] = np.exp2((r - s * B) // p)
        yield s, d


def decode_sparse_bwd(dws, fp, fi, p, sc):
    """dws: the dW [F, p] of every call of sparse_bwd_douts, in order -> keep [nnz]"""
    fp = np.asarray(fp, np.int64)
    rows = np.repeat(np.arange(fp.size - 1), np.diff(fp))
    cols = np.asarray(fi, np.int64)
    B = SPARSE_BWD_ROWS * p
    Ns = [_exact_int(np.asarray(dw, np.float64) / float(sc), "sparse weight gradient") for dw in dws]
    keep_bits = np.zeros(rows.size, bool)
    for s, N in enumerate(Ns):
        sel = rows // B == s
        i = rows[sel] - s * B
        keep_bits[sel] = ((N[cols[sel], i % p] >> (i // p)) & 1).astype(bool)
        assert int(N.sum()) == int(keep_bits[sel].astype(np.int64) @ (1 << (i // p))), "dW holds a term that no stored value explains"
    return keep_bits
