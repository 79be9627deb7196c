"""float64 numpy references of the element-wise layer (csrc/elementwise.hip: Adam, the sum of squares, ReLU / Dropout in their
strided forms; csrc/graphsum.hip: the bf16 converter), each with an ERROR BOUND derived from the kernel's operation order, so
that no tolerance has to be guessed — plus an f32 numpy emulation of adam_kernel's element update and variable selection, whose
mutants show (without a GPU) that the bounds reject a subtly wrong kernel.  No GPU code here; numpy only.

Notation: u = 2^-24 is the unit roundoff of f32 (one correctly rounded f32 operation on a real value x returns x (1 + d),
|d| <= u), eps_f32 = 2^-23 = 2 u, TINY = 2^-126 the smallest normal f32.  Every bound below is a sum of such first-order terms
times (1 + SLACK); SLACK = 1e-6 covers the second-order products (each propagated error is itself rounded again: a factor
1 + u on a term already inside the bound) and the roundings of the double operations (2^-53 each).  TINY is added to every
bound as its absolute floor: where a product or a result is subnormal its error is no longer relative, and whether the hardware
keeps subnormals is not what these tests are about.

Adam (adam_kernel, one element; w, g, m, v, beta1, beta2, eps, wd, step are f32 values read exactly; src/seq/optim.cpp:24-37):

    grad  = decay ? g + wd . w : g                          f32.  The compiler may contract the product into the sum (one
                                                            FMA, one rounding) or not (two roundings).  With G the real value:
                                                                d_G = u (|g| + 2 |wd . w|)      with decay, 0 without
                                                            (not contracted: u |wd w| for the product, u (|g| + |wd w|) for the
                                                            sum; contracted: u |G|, which is smaller)
    m'    = (float)((double)(beta1 . m) + (1.0 - beta1) . grad)
                                                            beta1 . m is ONE f32 product (rounded: u |beta1 m|); 1.0 - beta1,
                                                            its product with grad and the sum are doubles (an FMA there changes
                                                            2^-53); the narrowing rounds the sum once: u |M|
                                                                E_m = u (|beta1 m| + |M|) + (1 - beta1) d_G
    v'    = (float)((double)(beta2 . v) + (1.0 - beta2) . grad . grad)
                                                            the same shape; grad . grad is a DOUBLE product of the f32 grad, so
                                                            only d_G enters it: |grad^2 - G^2| <= 2 |G| d_G + d_G^2
                                                                E_v = u (|beta2 v| + V) + (1 - beta2) (2 |G| d_G + d_G^2)
                                                            A real V at or above (2 - 2^-24) 2^127 narrows to +inf: the
                                                            reference then says +inf with bound 0.
    w'    = w - step . m' / (sqrtf(v') + eps)                f32 throughout, from the STORED m', v' (f32 values, exact inputs of
                                                            this line).  p = step . m' rounds once (u); sqrtf is correctly
                                                            rounded (u) and its sum with eps rounds once: the divisor is within
                                                            2 u of D = sqrt(v') + eps (both terms are >= 0, so u sqrt(v') <= u D);
                                                            the division is correctly rounded (u): the quotient is within 4 u
                                                            of Q = step m' / D.  No contraction is possible (a quotient is
                                                            subtracted).  The difference rounds once: u |W|
                                                                E_w = u (|W| + 4 |Q|)
                                                            E_w is stated against the m', v' the implementation under test
                                                            stored (they are passed in): a wrong moment is reported as a wrong
                                                            moment, never as a wrong weight.  v' = +inf gives Q = 0 and W = w.
                                                            (hipcc's default is the correctly rounded f32 division and square
                                                            root; the build passes no flag that relaxes them.)
Each bound is thus at most 2.5 eps_f32 times the sum of the magnitudes of the terms that enter the value.

Sum of squares (sumsq_partial_kernel + sum_partials_kernel; adam_kernel's `sq` with either final sum): every term x^2 >= 0 is
rounded once (or contracted into its addition) and then goes through a chain of f32 additions of non-negative numbers, each of
which multiplies what it carries by at most (1 + u): after `depth` additions and the square's own rounding the result is within
((1 + u)^(depth + 1) - 1) sum x^2 <= (depth + 1) eps_f32 sum x^2 of the real sum (a TRUE relative bound: nothing cancels; eps_f32 =
2 u leaves the second-order terms far behind for any depth below 2^22).  depth is the longest path of the kernel's tree:
    per thread   ceil(min(chunk, n_terms) / 256) additions (256 threads stride the block's contiguous chunk)
    wave         6 (xor butterfly over 64 lanes)
    block        3 (sh[0] + sh[1] + sh[2] + sh[3])
    partials     ceil(blocks / 256) + 6 + 3 (one block strides the partials, then the same wave and block sums)

Strided ReLU / Dropout: element i = r . cols + c of the logical matrix lives at r . ld + c; masks, the injected keep decisions
and the dropout stream are keyed by i.  These are exact operations: the references return bit patterns."""
import numpy as np

U = 2.0 ** -24
EPS_F32 = 2.0 ** -23
TINY = 2.0 ** -126
SLACK = 1e-6
F32_OVERFLOW = (2.0 - 2.0 ** -24) * 2.0 ** 127        # a real number at or above this narrows to +inf (round to nearest even)
PAD_BITS = 0x7FC5A5A5                                 # the padding sentinel: a quiet NaN with a payload no operation produces

# Adam's hyper-parameters (beta1, beta2, eps, wd): the model's, and a set whose 1 - beta is NOT an f32 number (1 - 0.9f and
# 1 - 0.999f are: a kernel that forms them in float would pass unnoticed on the model's set alone)
HYPER_MODEL = (0.9, 0.999, 1e-8, 5e-4)
HYPER_INEXACT = (0.4, 0.4, 1e-8, 5e-4)

# (elements per variable, decay flags): the layouts of the GPU tests, by the edge they reach
LAYOUTS = [
    ([300], [1]),                                     # single variable
    ([1], [1]),                                       # one-element variable
    ([255, 1, 257], [0, 1, 0]),                       # boundaries inside a 256-thread group
    ([1000, 112, 7, 300], [1, 0, 1, 0]),              # four variables
    ([63, 65, 64, 64], [0, 0, 1, 1]),                 # boundaries inside a wave
    ([1024 * 1024 + 1], [1]),                         # block cap (1024 blocks of 1280) with empty trailing blocks
    ([1024 * 1024 - 5, 300], [1, 0]),                 # the second variable starts in the last used block
]
BOUNDARY_LAYOUT = ([300, 112], [1, 0])                # the layout on which an off-by-one variable boundary is shown rejected


def f32(x):
    """the f32 value nearest to x, as a Python float: what a kernel argument holds"""
    return float(np.float32(x))


def step_size(lr, beta1, beta2, t):
    """optim.cpp:26 in f32 arithmetic: lr . sqrtf(1 - powf(beta2, t)) / (1 - powf(beta1, t)).  powf is taken correctly rounded
    (the double power, narrowed), as the C library's is: 1 - powf(0.999f, t) cancels, and a power one bit off moves the step
    size by 3e-6 of itself"""
    one = np.float32(1)
    p1, p2 = np.float32(float(np.float32(beta1)) ** int(t)), np.float32(float(np.float32(beta2)) ** int(t))
    return float(np.float32(lr) * np.sqrt(one - p2) / (one - p1))


# ------------------------------------------------------------------------------------------------------------------ Adam
def adam_step_ref(w, g, m, v, decay, step, beta1, beta2, eps, wd, m_got=None, v_got=None):
    """One step from the f32 state (w, g, m, v) of one variable, in float64.  Returns ((w', m', v'), (E_w, E_m, E_v)): float64
    arrays and their per-element bounds (module docstring).  m_got, v_got: the m', v' the implementation under test stored — w'
    and E_w are stated against them (None: against the reference's own m', v' narrowed to f32).  v' is +inf, with bound 0, where
    the real value narrows to +inf."""
    w, g, m, v = (np.asarray(t, np.float32).astype(np.float64) for t in (w, g, m, v))
    b1, b2, e, wdec, st = f32(beta1), f32(beta2), f32(eps), f32(wd), f32(step)
    with np.errstate(over="ignore", invalid="ignore"):
        if decay:
            G = g + wdec * w
            d_g = U * (np.abs(g) + 2 * np.abs(wdec * w))
        else:
            G, d_g = g, np.zeros_like(g)
        M = b1 * m + (1.0 - b1) * G
        e_m = (U * (np.abs(b1 * m) + np.abs(M)) + (1.0 - b1) * d_g) * (1 + SLACK) + TINY
        V = b2 * v + (1.0 - b2) * G * G
        e_v = (U * (np.abs(b2 * v) + V) + (1.0 - b2) * (2 * np.abs(G) * d_g + d_g * d_g)) * (1 + SLACK) + TINY
        over = V >= F32_OVERFLOW
        V = np.where(over, np.inf, V)
        e_v = np.where(over, 0.0, e_v)
        ms = np.asarray(m_got, np.float32).astype(np.float64) if m_got is not None else M.astype(np.float32).astype(np.float64)
        vs = np.asarray(v_got, np.float32).astype(np.float64) if v_got is not None else V.astype(np.float32).astype(np.float64)
        Q = st * ms / (np.sqrt(vs) + e)
        W = w - Q
        e_w = U * (np.abs(W) + 4 * np.abs(Q)) * (1 + SLACK) + TINY
    return (W, M, V), (e_w, e_m, e_v)


def violation(got, want, bound):
    """max over the elements of |got - want| - bound (<= 0: inside), comparing infinities by equality (a bound of 0 there);
    NaN anywhere counts as +inf outside"""
    got, want, bound = (np.asarray(t, np.float64).ravel() for t in (got, want, bound))
    assert got.shape == want.shape == bound.shape, (got.shape, want.shape, bound.shape)
    if got.size == 0:
        return -np.inf
    inf = np.isinf(want)
    with np.errstate(invalid="ignore"):
        d = np.where(inf, np.where(got == want, 0.0, np.inf), np.abs(got - want)) - bound
    return float(np.where(np.isnan(d), np.inf, d).max())


def adam_violations(w, g, m, v, decay, step, hyper, got_w, got_m, got_v):
    """(viol_w, viol_m, viol_v) of one variable's result (got_*) against adam_step_ref from the state (w, g, m, v)"""
    (W, M, V), (ew, em, ev) = adam_step_ref(w, g, m, v, decay, step, *hyper, m_got=got_m, v_got=got_v)
    return violation(got_w, W, ew), violation(got_m, M, em), violation(got_v, V, ev)


def adam_state(layout, seed, scale_m=0.1):
    """random f32 state of the variables of a layout: (ws, gs, ms, vs), m non-zero and v >= 0"""
    rng = np.random.default_rng(seed)
    out = ([], [], [], [])
    for n in layout:
        out[0].append(rng.standard_normal(n).astype(np.float32))
        out[1].append(rng.standard_normal(n).astype(np.float32))
        out[2].append((rng.standard_normal(n) * scale_m).astype(np.float32))
        out[3].append(((rng.standard_normal(n) * scale_m) ** 2).astype(np.float32))
    return out


def adam_edge_states(n=67, seed=11):
    """name -> (w, g, m, v, decay, hyper): the edge values of the GPU tests, each on its own small array of one variable.
    zero: g = m = v = 0 (w' = w);  double_square: g = 1e20, whose square only a double holds ((1 - beta2) g^2 ~ 1e37 is an
    f32 again);  overflow: g = 1e21, (1 - beta2) g^2 ~ 1e39 narrows to +inf, and w' = w - step m' / inf = w;  no_wd: wd = 0"""
    (w,), (g,), (m,), (v,) = adam_state([n], seed)
    z = np.zeros(n, np.float32)
    b1, b2, eps, _ = HYPER_MODEL
    sign = np.where(np.arange(n) % 2 == 0, 1, -1).astype(np.float32)
    return {
        "zero": (w, z, z, z, 0, HYPER_MODEL),
        "double_square": (w, (np.float32(1e20) * sign).astype(np.float32), m, v, 1, HYPER_MODEL),
        "overflow": (w, (np.float32(1e21) * sign).astype(np.float32), m, v, 0, HYPER_MODEL),
        "no_wd": (w, g, m, v, 1, (b1, b2, eps, 0.0)),
    }


def adam_grid(total):
    """(blocks, chunk) of adam_step_impl / adam_kernel for `total` fused elements"""
    blocks = min(max((total + 1023) // 1024, 1), 1024)
    chunk = ((total + blocks - 1) // blocks + 255) // 256 * 256
    return blocks, chunk


def sumsq_grid(n):
    """(blocks, chunk) of gcnhip_sumsq / sumsq_partial_kernel for n elements"""
    blocks = min(max((n + 4095) // 4096, 1), 1024)
    chunk = ((n + blocks - 1) // blocks + 255) // 256 * 256
    return blocks, chunk


def sumsq_depth(n_terms, blocks, chunk):
    """additions on the longest path from a term to the result (module docstring)"""
    per_thread = (min(chunk, max(n_terms, 1)) + 255) // 256
    return per_thread + 6 + 3 + (blocks + 255) // 256 + 6 + 3


def sumsq_bound(n_terms, blocks, chunk, sum_sq=1.0):
    """(depth + 1) . eps_f32 . sum x^2: how far the kernels' f32 sum of n_terms squares, `blocks` blocks of `chunk` contiguous
    elements each, may lie from the real sum `sum_sq` (1.0: the relative bound)"""
    return (sumsq_depth(n_terms, blocks, chunk) + 1) * EPS_F32 * sum_sq


def sumsq_f64(x):
    return float((np.asarray(x, np.float32).astype(np.float64) ** 2).sum())


MUTANTS = ("float_square", "float_one_minus_beta", "decay_wrong_variable", "boundary_off_by_one", "table_index_zero",
           "sumsq_all_variables", "m_from_new_v")


def adam_kernel_emul(ws, gs, ms, vs, decays, step, hyper, table=None, epoch=0, mutant=None):
    """adam_kernel in f32 numpy, element by element as the kernel orders it: the variables are laid end to end in the fused
    index space, `start[]` holds their offsets, variable k of fused index i is the last q with i >= start[q], and that variable's
    decay flag applies.  step: the scalar step size, unless `table` is given (then table[epoch], as d_step_sizes[*d_epoch]).
    Returns (ws', ms', vs', sumsq): per variable f32 arrays and the float64 sum of w'^2 over variable 0's elements (the kernel's
    `if (k == 0)`), to be held against sumsq_bound.  The product of the decay is not contracted here; the kernel's may be (d_G
    covers both).  mutant: one of MUTANTS — a subtly wrong kernel."""
    assert mutant is None or mutant in MUTANTS
    beta1, beta2, eps, wd = (np.float32(t) for t in hyper)
    n_vars = len(ws)
    sizes = [int(np.asarray(t).size) for t in ws]
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    w, g, m, v = (np.concatenate([np.asarray(t, np.float32).ravel() for t in ts]) for ts in (ws, gs, ms, vs))
    i = np.arange(start[-1], dtype=np.int64)
    k = np.zeros(i.size, np.int64)
    for q in range(1, 4):
        if q < n_vars:
            k = np.where((i > start[q]) if mutant == "boundary_off_by_one" else (i >= start[q]), q, k)
    flags = np.asarray(decays, np.int64) != 0
    if mutant == "decay_wrong_variable":
        flags = np.roll(flags, 1)
    if table is not None:
        step = np.asarray(table, np.float32)[0 if mutant == "table_index_zero" else int(epoch)]
    step = np.float32(step)
    one = np.float32(1)
    if mutant == "float_one_minus_beta":
        omb1, omb2 = float(one - beta1), float(one - beta2)
    else:
        omb1, omb2 = 1.0 - float(beta1), 1.0 - float(beta2)
    with np.errstate(over="ignore", invalid="ignore"):
        grad = np.where(flags[k], g + wd * w, g).astype(np.float32)
        gd = grad.astype(np.float64)
        sq = (grad * grad).astype(np.float64) if mutant == "float_square" else gd * gd
        v_new = ((beta2 * v).astype(np.float64) + omb2 * sq).astype(np.float32)
        m_old = v_new if mutant == "m_from_new_v" else m
        m_new = ((beta1 * m_old).astype(np.float64) + omb1 * gd).astype(np.float32)
        w_new = (w - step * m_new / (np.sqrt(v_new) + eps)).astype(np.float32)
        counted = np.ones(i.size, bool) if mutant == "sumsq_all_variables" else k == 0
        sumsq = float((w_new[counted].astype(np.float64) ** 2).sum())
    cut = lambda a: [a[start[q]:start[q + 1]] for q in range(n_vars)]      # noqa: E731
    return cut(w_new), cut(m_new), cut(v_new), sumsq


# ------------------------------------------------------------------------------------------------- ReLU / Dropout, exact
def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def padded(data, ld, pad_bits=PAD_BITS):
    """[rows, cols] f32 -> [rows, ld] whose padding columns hold the sentinel bit pattern"""
    data = np.ascontiguousarray(data, np.float32)
    out = np.full((data.shape[0], ld), pad_bits, np.uint32)
    out[:, :data.shape[1]] = data.view(np.uint32)
    return out.view(np.float32)


def relu_fwd_ref(x):
    """flat: (y, mask uint8) — kept values unchanged, everything not > 0 (negatives, -0.0, NaN) becomes +0.0"""
    x = np.asarray(x, np.float32).ravel()
    with np.errstate(invalid="ignore"):
        keep = x > 0
    return np.where(keep, x, np.float32(0)).astype(np.float32), keep.astype(np.uint8)


def relu_bwd_ref(g, mask):
    g = np.asarray(g, np.float32).ravel()
    return np.where(np.asarray(mask).ravel() != 0, g, np.float32(0)).astype(np.float32)


def dropout_fwd_ref(x, keep, scale):
    """flat: x . (keep ? scale : 0) in f32 (NaN stays NaN, -0.0 . scale = -0.0), and the int32 mask"""
    x = np.asarray(x, np.float32).ravel()
    keep = np.asarray(keep).ravel() != 0
    with np.errstate(invalid="ignore"):
        y = x * np.where(keep, np.float32(scale), np.float32(0)).astype(np.float32)
    return y.astype(np.float32), keep.astype(np.int32)


def dropout_bwd_ref(g, mask, scale):
    return dropout_fwd_ref(g, mask, scale)[0]


def _apply_2d(buf, cols, fn):
    """run a flat reference on the logical [rows, cols] matrix inside buf [rows, ld]; every padding word keeps its bits"""
    buf = np.array(buf, np.float32, copy=True)
    out = fn(np.ascontiguousarray(buf[:, :cols]).ravel())
    flat, rest = (out[0], out[1:]) if isinstance(out, tuple) else (out, ())
    buf.view(np.uint32)[:, :cols] = bits(flat).reshape(buf.shape[0], cols)
    return (buf,) + tuple(rest) if rest else buf


def relu_fwd_2d_ref(buf, cols):
    """(buffer [rows, ld], mask uint8 [rows . cols] keyed by r . cols + c)"""
    return _apply_2d(buf, cols, relu_fwd_ref)


def relu_bwd_2d_ref(buf, cols, mask):
    return _apply_2d(buf, cols, lambda g: relu_bwd_ref(g, mask))


def dropout_fwd_2d_ref(buf, cols, keep, scale):
    """keep: decisions keyed by r . cols + c -> (buffer, int32 mask [rows . cols])"""
    return _apply_2d(buf, cols, lambda x: dropout_fwd_ref(x, keep, scale))


def dropout_bwd_2d_ref(buf, cols, mask, scale):
    return _apply_2d(buf, cols, lambda g: dropout_bwd_ref(g, mask, scale))


def relu_dropout_bwd_ref(gbuf, hbuf, dim, scale):
    """where(h > 0, g . scale, 0) on the first `dim` columns of gbuf [rows, ld_grad], h read from hbuf [rows, ld_h]"""
    gbuf = np.array(gbuf, np.float32, copy=True)
    g, h = gbuf[:, :dim], np.asarray(hbuf, np.float32)[:, :dim]
    with np.errstate(invalid="ignore"):
        out = np.where(h > 0, g * np.float32(scale), np.float32(0)).astype(np.float32)
    gbuf.view(np.uint32)[:, :dim] = out.view(np.uint32)
    return gbuf


def same_bits_or_nan(got, want):
    """bit-identical, except that where `want` is NaN any NaN will do (a product with NaN may quiet it)"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and bool(np.all(np.isnan(got[nan]))) and np.array_equal(bits(got)[~nan], bits(want)[~nan])


# ------------------------------------------------------------------------------------------------------------------ bf16
# (f32 bit pattern, bf16 code or None = "a NaN code with this sign"): the special values of the converter's tests
BF16_SPECIALS = [
    (0x7F800000, 0x7F80),          # +inf
    (0xFF800000, 0xFF80),          # -inf
    (0x80000000, 0x8000),          # -0.0
    (0x7F7FFFFF, 0x7F80),          # the largest finite f32 rounds to +inf under nearest-even
    (0xFF7FFFFF, 0xFF80),
    (0x00000001, 0x0000),          # the smallest subnormal
    (0x7FA00000, None),            # a signalling NaN
    (0xFFA00000, None),
    (0x7FC00000, None),            # a quiet NaN
    (0xFFC00001, None),
    (0x7F800001, None),            # a NaN whose top 16 bits alone read as +inf
    (0xFF800001, None),
    (0x3F808000, 0x3F80),          # 1 + 2^-8: a tie, down to the even code
    (0x3F818000, 0x3F82),          # 1 + 3 . 2^-8: a tie, up to the even code
    (0xBF808000, 0xBF80),
    (0xBF818000, 0xBF82),
]


def bf16_ref(x):
    """uint16 codes of f32 -> bf16, round to nearest even; NaN -> its top 16 bits with the quiet bit set (sign and the upper
    payload kept)"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    rne = ((u.astype(np.uint64) + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = ((u & 0x7F800000) == 0x7F800000) & ((u & 0x007FFFFF) != 0)
    return np.where(nan, ((u >> 16) | 0x40).astype(np.uint16), rne)


def bf16_is_nan(code):
    code = np.asarray(code, np.uint16)
    return ((code & 0x7F80) == 0x7F80) & ((code & 0x007F) != 0)
