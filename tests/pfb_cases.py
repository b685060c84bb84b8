"""The polyphase bank's kernel-selection rule, restated, and the case tables built on it.

PolyPhaseFilterBank and InterpolatingFIRFilter run on three kernel templates
(csrc/sdsp_pfb_walk.hpp): interp_tile_kernel<C, I, EXACT, K> for K = 4, 8, 16, pfb_stage_kernel<C, I,
EXACT, CB_LDS> and pfb_kernel<C, I, EXACT>; pfb_route picks one per call.  With the identity store
hook that is 6 type pairs x 6 kernels x 2 summation orders = 72 instantiations.  The handle cannot
say which one a call got (the bank has no info()), so the tests name it from this restatement: every
function below gives the lines of csrc/ it restates, and a reader has to hold the two side by side.
No GPU import: the CPU suite counts the instantiations and checks the tables and their inputs
(tests/test_pfb_cases.py), the GPU suite runs them (tests/test_gpu_pfb_paths.py).
"""
from __future__ import annotations

import collections

import numpy as np

F32, F64, C64, C128 = np.float32, np.float64, np.complex64, np.complex128

# name -> (sdsp dtype code, coef dtype, sample dtype, code of the 64-bit pair of the f64 restatement)
# (the codes are include/sdsp.h's and oracle_lib's: RR32 .. CC64 = 0 .. 5)
PAIRS = {
    "RR32": (0, F32, F32, 3), "RC32": (1, F32, C64, 4), "CC32": (2, C64, C64, 5),
    "RR64": (3, F64, F64, 3), "RC64": (4, F64, C128, 4), "CC64": (5, C128, C128, 5),
}
KERNELS = ("tile4", "tile8", "tile16", "staged_lds", "staged_global", "per_output")
ORDERS = ("exact", "fma")
K_STAGE_BYTES = 48 * 1024  # kPfbStageBytes, sdsp_pfb_walk.hpp:93
K_INTERP_R = 16            # kInterpR, :149


def code_of(pair):
    return PAIRS[pair][0]


def coef_dt(pair):
    return PAIRS[pair][1]


def sample_dt(pair):
    return PAIRS[pair][2]


def wide_code(pair):
    return PAIRS[pair][3]


def sample_bytes(pair):
    return np.dtype(PAIRS[pair][2]).itemsize


def coef_bytes(pair):
    return np.dtype(PAIRS[pair][1]).itemsize


def is_32bit(pair):
    return PAIRS[pair][0] <= 2


def tol_of(pair):
    """section 8d: 1e-6 for 32-bit samples, 1e-13 for 64-bit"""
    return 1e-6 if is_32bit(pair) else 1e-13


def wide(dt):
    return C128 if np.dtype(dt).kind == "c" else F64


# ---------------------------------------------------------------- the rule
def interp_k(L, M):
    """sdsp_interp_create, runtime.cpp:938-939: the quotient in f32, its ceiling unless it is whole
    (the taps are then zero-padded to K M, :941-942)"""
    q = F32(L) / F32(M)
    return int(q) if q == np.floor(q) else int(np.ceil(q))


def pfb_k(L, M):
    """pfb_create_common, runtime.cpp:867: K = floor(len / M); taps beyond K M are never read (:884-886)"""
    return L // M


def k_of(ctor, L, M):
    return interp_k(L, M) if ctor == "interp" else pfb_k(L, M)


def handle_taps(ctor, h, M):
    """the K M taps the handle keeps: zero-padded (interp, runtime.cpp:941-942) or cut (pfb, :884-886)"""
    K = k_of(ctor, len(h), M)
    out = np.zeros(K * M, h.dtype)
    n = min(len(h), K * M)
    out[:n] = h[:n]
    return out


def tile_geometry(M):
    """interp_tile_kernel, sdsp_pfb_walk.hpp:165: P lanes per run, G runs per workgroup, T inputs per tile"""
    P = M // 2
    G = 256 // P
    return P, G, G * K_INTERP_R


def interp_tile_applies(pair, M, K, H, offset):
    """interp_tile_applies, sdsp_pfb_walk.hpp:209-212.  offset: samples the output sits past an
    allocation aligned to two samples or more"""
    sb = sample_bytes(pair)
    return (8 <= M <= 512 and M & (M - 1) == 0 and K in (4, 8, 16) and H == K and
            (offset * sb) % (2 * sb) == 0)


def pfb_route(pair, M, K):
    """pfb_route, sdsp_pfb_walk.hpp:240-243: (T, xb, cbb, staged, cb_lds)"""
    T = 1 if M >= 4096 else 4096 // M
    xb = ((T + K - 1) * sample_bytes(pair) + 15) // 16 * 16
    cbb = M * K * coef_bytes(pair)
    staged = xb <= K_STAGE_BYTES and T * M < (1 << 31)
    return T, xb, cbb, staged, staged and xb + cbb <= K_STAGE_BYTES


def kernel_of_k(pair, M, K, offset=0, H=None):
    """the kernel pfb_route launches for a bank of M branches of K taps, sdsp_pfb_walk.hpp:217-269.
    H is the history the call reads: K in execute_block (runtime.cpp:1007), K - 1 in execute(idx)
    (:1044-1045)"""
    if interp_tile_applies(pair, M, K, K if H is None else H, offset):
        return f"tile{K}"
    _, _, _, staged, cb_lds = pfb_route(pair, M, K)
    if staged:
        return "staged_lds" if cb_lds else "staged_global"
    return "per_output"


def kernel_of(pair, ctor, L, M, offset=0, H=None):
    """ctor: "interp" (InterpolatingFIRFilter) or "pfb" (PolyPhaseFilterBank) of L taps"""
    return kernel_of_k(pair, M, k_of(ctor, L, M), offset, H)


def instantiations():
    """every (pair, kernel, order) of the identity store hook"""
    return [(p, k, o) for p in PAIRS for k in KERNELS for o in ORDERS]


# ---------------------------------------------------------------- the shapes
BOTH = ("interp", "pfb")
ALL = tuple(PAIRS)
S4, S8, S16 = ("RR32",), ("RC32", "CC32", "RR64"), ("RC64", "CC64")

# (L, M, pairs, constructors, kernel).  The smallest shapes that reach each instantiation:
SHAPES = (
    # tile: every corner of M in {8, 32, 512} x K in {4, 8, 16}.  M = 8 fills xs[] to 1024 + K - 1
    # entries (1039 of 1040 at K = 16), M = 512 has one run per workgroup (G = 1, T = 16)
    [(M * K, M, ALL, BOTH, f"tile{K}") for M in (8, 32, 512) for K in (4, 8, 16)] +
    # 60 taps on 16 branches: the interpolator pads to K = 4, the bank drops 12 taps for K = 3
    [(60, 16, ALL, ("interp",), "tile4"), (60, 16, ALL, ("pfb",), "staged_lds")] +
    # staged, branch taps in LDS: T = 1024, 1365, 4096, 585, 4 inputs per workgroup
    [(10, 4, ALL, BOTH, "staged_lds"), (9, 3, ALL, BOTH, "staged_lds"), (5, 1, S4 + S8, BOTH, "staged_lds"),
     (7, 7, ALL, BOTH, "staged_lds"), (3000, 1000, ALL, BOTH, "staged_lds")] +
    # staged, branch taps in global memory: M K sizeof(coef) = 51200 > 48 KiB with K = 100 or 50
    [(12800, 128, ("RR32", "RC32"), BOTH, "staged_global"),
     (6400, 64, ("CC32", "RR64", "RC64"), BOTH, "staged_global"),
     (3200, 64, ("CC64",), BOTH, "staged_global"),
     # T + K - 1 = 3072 16-byte samples: xb is 48 KiB to the byte, the staged kernel's last shape
     (2050, 2, S16, BOTH, "staged_global")] +
    # per output: the first shapes past 48 KiB of staged samples at M = 1 and M = 2
    [(5, 1, S16, BOTH, "per_output"), (2052, 2, S16, BOTH, "per_output"),
     (2050, 1, S8, BOTH, "per_output"), (8196, 2, S8, BOTH, "per_output"),
     (8194, 1, S4, BOTH, "per_output"), (20484, 2, S4, BOTH, "per_output")]
)

Case = collections.namedtuple("Case", "pair ctors L M kernel order")


def case_id(c):
    return f"{c.pair}-L{c.L}-M{c.M}-{'+'.join(c.ctors)}-{c.kernel}-{c.order}"


def cases(order, kernels=KERNELS):
    """one case per (shape, pair) in `order`, restricted to `kernels`"""
    return [Case(pair, ctors, L, M, kern, order)
            for L, M, pairs, ctors, kern in SHAPES for pair in pairs if kern in kernels]


EXACT_CASES = cases("exact")
FMA_CASES = cases("fma")
# the impulse test: every fused case, and the reference order where the branches are long
IMPULSE_CASES = FMA_CASES + cases("exact", ("staged_global", "per_output"))

# one order, three kernels: (L, M) per tile kernel, on every pair and order
THREE_KERNEL_SHAPES = [(128, 32), (256, 32), (512, 32)]


def channel_shape(pair, kernel):
    """the shape of the three-channel test for a pair and kernel family"""
    if kernel == "tile16":
        return 128, 8
    if kernel == "staged_lds":
        return 9, 3
    rows = [(L, M) for L, M, pairs, _, kern in SHAPES if kern == kernel and pair in pairs and M > 1]
    return rows[0]


CHANNEL_PAIRS = ("RR32", "CC32", "RC64")  # 4-, 8- and 16-byte samples
CHANNEL_KERNELS = ("tile16", "staged_lds", "staged_global", "per_output")
CHANNEL_CASES = [Case(p, ("interp",), *channel_shape(p, k), k, o)
                 for p in CHANNEL_PAIRS for k in CHANNEL_KERNELS for o in ORDERS]

# pfb_kernel's grid holds at most 65536 workgroups of 256 lanes (sdsp_pfb_walk.hpp:260-261): past
# that many outputs a lane takes a second turn
GRID_STRIDE_N = 65536 * 256 + 777


# ---------------------------------------------------------------- the streams
RAGGED = (0, 1, 1, 1028, 1, 1970, 0, 777)  # tile and run boundaries inside calls, history read
LONG_K = 1000  # from here on a case counts as long: short calls, sparse taps on 32-bit pairs


def calls_of(K):
    """the calls of a white-input stream.  Long branches get calls of at most 300 inputs, as many as
    it takes to fill the history, so that every tap has met data before the stream ends.  They have
    M = 1 or 2, so none of their calls is a single input: the rel-RMS of a call of one or two
    outputs is the relative error of a single sum of thousands of terms, which cancellation leaves
    unbounded at any precision (the f32 restatement itself: 7.8e-6 on one such output)"""
    if K < LONG_K:
        return RAGGED
    return (0, 300, 257, 0, 77) + (300,) * (-(-K // 300)) + (211,)


def spans(calls):
    at, out = 0, []
    for n in calls:
        out.append((at, at + n))
        at += n
    return out


# ---------------------------------------------------------------- inputs
def white_taps(L, cdt, seed):
    """white taps of variance 1 / L per component (Kaiser taps hide dropped end taps)"""
    r = np.random.default_rng(seed)
    h = r.standard_normal(L)
    if np.dtype(cdt).kind == "c":
        h = h + 1j * r.standard_normal(L)
    return (h / np.sqrt(L)).astype(cdt)


def sparse_taps(L, M, cdt, seed):
    """long branches on 32-bit pairs: per branch 64 white taps at its start, 64 in its middle and 64
    at its end, of variance 1 / 192, zeros elsewhere (a zero tap leaves the accumulator as it is in
    both summation orders, so a sequential f32 sum stays fair to section 8d)"""
    K = L // M
    assert K * M == L and K >= 192
    idx = np.concatenate([np.arange(64), K // 2 - 32 + np.arange(64), K - 64 + np.arange(64)])
    dense = white_taps(192 * M, cdt, seed).reshape(192, M) * cdt(np.sqrt(M))
    h = np.zeros((K, M), cdt)
    h[idx] = dense  # h[idx * M + p]: tap idx of branch p
    return h.reshape(-1)


def white_input(n, sdt, seed):
    r = np.random.default_rng(seed)
    x = r.standard_normal(n)
    if np.dtype(sdt).kind == "c":
        x = x + 1j * r.standard_normal(n)
    return x.astype(sdt)


def taps_of(pair, L, M, dense=False):
    """the taps of a case at the handle's precision, read-only: white, or sparse white where a
    fused kernel is held to section 8d on long branches in f32"""
    seed = 3000 + 11 * L + M + code_of(pair)
    if not dense and is_32bit(pair) and L // M >= LONG_K:
        h = sparse_taps(L, M, coef_dt(pair), seed)
    else:
        h = white_taps(L, coef_dt(pair), seed)
    h.setflags(write=False)
    return h


def white_case(c):
    """(taps, calls, white stream) of a case; the taps are dense in the reference order, which is
    held to no tolerance"""
    K = k_of(c.ctors[0], c.L, c.M)
    calls = calls_of(K)
    x = white_input(sum(calls), sample_dt(c.pair), 4000 + c.M + code_of(c.pair))
    x.setflags(write=False)
    return taps_of(c.pair, c.L, c.M, dense=c.order == "exact"), calls, x


def impulse_amp(pair):
    sdt = sample_dt(pair)
    return sdt(0.5 - 0.25j) if np.dtype(sdt).kind == "c" else sdt(0.5)


def impulse_case(c):
    """(taps, calls, stream, impulse positions).  Zero input but for impulses more than K inputs
    apart: at the stream's first input, at the last input of the first call (the response runs on
    through the history), before a tile boundary of the second call (the tile kernel's T or the
    staged kernel's) and, for the tile kernel, before a run boundary that is no tile boundary
    (with one run per tile, M = 512, a second tile boundary)"""
    K = k_of(c.ctors[0], c.L, c.M)
    n1 = K + 2
    pos2 = []
    if c.kernel.startswith("tile"):
        T = tile_geometry(c.M)[2]
    elif c.kernel.startswith("staged"):
        T = pfb_route(c.pair, c.M, K)[0]
    else:
        T = 0
    at = K  # the first input of call 2 that is clear of call 1's last response
    if T:
        b = (at + T) // T * T - 1
        pos2.append(b)
        at = b + K + 1
        if c.kernel.startswith("tile"):
            r = (at + K_INTERP_R) // K_INTERP_R * K_INTERP_R - 1
            if T > K_INTERP_R and (r + 1) % T == 0:
                r += K_INTERP_R
            pos2.append(r)
            at = r + K + 1
    n2 = at + 1
    pos = [0, n1 - 1] + [n1 + p for p in pos2]
    x = np.zeros(n1 + n2, sample_dt(c.pair))
    x[pos] = impulse_amp(c.pair)
    x.setflags(write=False)
    h = white_taps(c.L, coef_dt(c.pair), 5000 + 11 * c.L + c.M + code_of(c.pair))
    h.setflags(write=False)
    return h, (n1, n2), x, pos


def response_mask(n, M, K, pos):
    """True at every output of a stream of n inputs that lies inside an impulse's response"""
    m = np.zeros((n, M), bool)
    for p in pos:
        m[p:p + K] = True
    return m.reshape(-1)


# ---------------------------------------------------------------- section 8d
def bound_8d(pair, h, x):
    """tol * sum|h| * max|x|"""
    return tol_of(pair) * float(np.sum(np.abs(h.astype(C128)))) * float(np.max(np.abs(x)))


def measure_8d(y, ref):
    y = np.asarray(y, dtype=C128)
    ref = np.asarray(ref, dtype=C128)
    assert y.shape == ref.shape, (y.shape, ref.shape)
    rr = float(np.linalg.norm(y - ref) / max(np.linalg.norm(ref), 1e-300))
    ma = float(np.max(np.abs(y - ref))) if y.size else 0.0
    return rr, ma


def check_8d(pair, y, ref, h, x, what, share=1.0, quiet=False):
    """both criteria at `share` of the tolerance: rel-RMS <= share tol and max-abs <= share tol
    sum|h| max|x|; returns (rel-RMS, max-abs as a share of the whole bound)"""
    rr, ma = measure_8d(y, ref)
    bound = bound_8d(pair, h, x)
    if not quiet:
        print(f"{what}: rel-RMS {rr:.3e} max-abs {ma:.3e} (bound {bound:.3e}, {ma / bound:.4f} of it)")
    assert rr <= share * tol_of(pair), (what, rr)
    assert ma <= share * bound, (what, ma, bound)
    return rr, ma / bound


def check_stream_8d(pair, y, ref, h, x, M, calls, what, share=1.0):
    """section 8d per call and over the whole stream; the worst (rel-RMS, share of the bound)"""
    worst = check_8d(pair, y, ref, h, x, what, share)
    for a, b in spans(calls):
        if b > a:
            f = check_8d(pair, y[a * M:b * M], ref[a * M:b * M], h, x[:b], f"{what} [{a}, {b})", share, quiet=True)
            worst = (max(worst[0], f[0]), max(worst[1], f[1]))
    return worst


# ---------------------------------------------------------------- shapes of an existing test
# test_pfb_staged_kernel_bit_parity (tests/test_gpu_fir.py) runs PolyPhaseFilterBank on these (L, M)
STAGED_PARITY_SHAPES = [(21, 3), (240, 24), (3000, 1000), (6000, 2), (12000, 2)]
