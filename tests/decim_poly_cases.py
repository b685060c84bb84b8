"""The polyphase decimator's dispatch rule and geometry, restated, and the case table built on it.

decim_poly_kernel<C, I, M, K, V> (csrc/kern_decim.hip) is what ALGO_FMA runs on a decimating handle
whose shape is "on the rule".  The handle cannot say which instantiation a call got (the decimator
has no info()), so the tests name it from this restatement: every function below gives the line of
csrc/ it restates, and a reader has to hold the two side by side.  No GPU import: the CPU suite
counts the instantiations and checks the coverage of the GPU cases (tests/test_decim_poly_cases.py),
the GPU suite runs them (tests/test_gpu_decim_poly.py).
"""
from __future__ import annotations

import functools

import numpy as np

F32, F64, C64, C128 = np.float32, np.float64, np.complex64, np.complex128

# name -> (sdsp dtype code, coef dtype, sample dtype, code of the 64-bit pair of the f64 restatement)
# (the codes are include/sdsp.h's and oracle_lib's: RR32 .. CC64 = 0 .. 5)
PAIRS = {
    "RR32": (0, F32, F32, 3), "RC32": (1, F32, C64, 4), "CC32": (2, C64, C64, 5),
    "RR64": (3, F64, F64, 3), "RC64": (4, F64, C128, 4), "CC64": (5, C128, C128, 5),
}
MS, KS = (8, 16, 32, 64), (2, 4, 8, 16)
K_POLY_WAVES = 4  # sdsp_decim_walk.hpp:84-85, kPolyThreads / 64


def sample_bytes(pair):
    return np.dtype(PAIRS[pair][2]).itemsize


def is_32bit(pair):
    return PAIRS[pair][0] <= 2


def tol_of(pair):
    """section 8d: 1e-6 for 32-bit samples, 1e-13 for 64-bit"""
    return 1e-6 if is_32bit(pair) else 1e-13


# ---------------------------------------------------------------- the rule
def on_rule(pair, L, M, fma=True):
    """try_launch_decim_poly, kern_decim.hip:129-130 (not exact, M >= 8, L % M == 0); poly_by_m
    :114-123 (M in {8, 16, 32, 64} with an M-sample row of 32..256 bytes); poly_by_k :103-111
    (L / M in {2, 4, 8, 16})"""
    if not fma or M < 8 or L % M != 0:
        return False
    if M not in MS or not 32 <= M * sample_bytes(pair) <= 256:
        return False
    return L // M in KS


def vector_width(pair):
    """VW of poly_by_v, kern_decim.hip:91: samples in 16 bytes, 1 for a 16-byte sample"""
    sz = sample_bytes(pair)
    return 1 if sz >= 16 else 16 // sz


def lane_width(pair, j0, n, channels, ptr_aligned):
    """poly_by_v, kern_decim.hip:92-99: V = VW when VW > 1, every row start is a multiple of VW
    ((j0 + 1) % VW == 0), the channel bases keep the alignment (one channel, or n % VW == 0) and the
    input pointer is a multiple of 16 bytes; else one sample per lane"""
    vw = vector_width(pair)
    if vw > 1 and (j0 + 1) % vw == 0 and (channels == 1 or n % vw == 0) and ptr_aligned:
        return vw
    return 1


def j0_of(M, ci):
    """FirCore::j0, sdsp_host.hpp:340: the first input index whose push wraps the phase to 0"""
    return (M - 1 - ci) % M


def output_count(M, ci, n):
    """FirCore::output_count, sdsp_host.hpp:341-344"""
    j0 = j0_of(M, ci)
    return (n - 1 - j0) // M + 1 if j0 < n else 0


def geometry(pair, M, K, V):
    """PolyGeom<I, M, K, V>, sdsp_decim_walk.hpp:87-92, and SPC of poly_group, :106:
    (MV lanes per group, G groups per wave, CH rows per reduction chunk, P lanes per output in the
    reduction, RPL outputs per lane when CH >= MV, SPC K-row steps per chunk)"""
    MV = M // V
    G = 64 // MV
    CH = K if K > MV // 4 else MV // 4
    P = MV // CH if MV > CH else 1
    RPL = CH // MV if CH > MV else 1
    return MV, G, CH, P, RPL, CH // K


def poly_seg(seg_arg, nout, CH):
    """poly_seg, sdsp_decim_walk.hpp:195-201: outputs per lane group, a multiple of CH"""
    seg = seg_arg if seg_arg > 0 else (nout + 8191) // 8192
    if seg_arg <= 0 and seg > 256:
        seg = 256
    seg = (seg + CH - 1) // CH * CH
    return max(seg, CH)


def waves_of(pair, M, K, V, nout, seg_arg):
    """launch_poly_t, kern_decim.hip:77-79: (seg, groups, waves) of a call"""
    _, G, CH, _, _, _ = geometry(pair, M, K, V)
    seg = poly_seg(seg_arg, nout, CH)
    groups = (nout + seg - 1) // seg
    return seg, groups, (groups + G - 1) // G


def instantiations():
    """every (pair, M, K, V) the dispatch can reach"""
    out = []
    for pair in PAIRS:
        for M in MS:
            for K in KS:
                if on_rule(pair, M * K, M):
                    out += [(pair, M, K, V) for V in sorted({1, vector_width(pair)})]
    return out


# every (pair, M, K) on the rule
SHAPES = [(pair, M, K) for pair in PAIRS for M in MS for K in KS if on_rule(pair, M * K, M)]


def geometry_shapes():
    """one (pair, M, K, V) per distinct geometry, taken in turn from the instantiations that have it
    so that every pair appears"""
    by_geo = {}
    for inst in instantiations():
        by_geo.setdefault(geometry(*inst), []).append(inst)
    return [lst[(5 * i) % len(lst)] for i, lst in enumerate(by_geo.values())]


# ---------------------------------------------------------------- the streams
# three calls.  N1 = 4 mod every M: the second call starts at phase 4 with j0 + 1 = M - 4, still a
# multiple of every VW; 4 + N2 is odd, so the third starts at an odd phase and takes one sample per
# lane whatever the pointer
CALLS = (98308, 40001, 20003)
SEG = 32  # SDSP_TUNE_DECIM_SEG of the stream cases: a multiple of every CH


def call_plan(pair, M, offset, calls=CALLS, channels=1):
    """[(n, phase before, j0, nout, V)] of a fresh handle's calls, the input `offset` samples past a
    16-byte aligned allocation"""
    plan, ci = [], 0
    aligned = (offset * sample_bytes(pair)) % 16 == 0
    for n in calls:
        j0 = j0_of(M, ci)
        plan.append((n, ci, j0, output_count(M, ci, n), lane_width(pair, j0, n, channels, aligned)))
        ci = (ci + n) % M
    return plan


def stream_cases():
    """(pair, M, K, offset, lane widths of the three calls) for every shape and both alignments"""
    return [(pair, M, K, offset, tuple(c[4] for c in call_plan(pair, M, offset)))
            for pair, M, K in SHAPES for offset in (0, 1)]


def case_id(pair, M, K, offset, widths):
    return f"{pair}-M{M}-K{K}-{'offset1' if offset else 'aligned'}-v{'.'.join(map(str, widths))}"


# ---------------------------------------------------------------- inputs
def white_taps(L, coef_dt, seed):
    """white taps of variance 1 / L per component (Kaiser taps hide dropped end taps)"""
    r = np.random.default_rng(seed)
    h = r.standard_normal(L)
    if np.dtype(coef_dt).kind == "c":
        h = h + 1j * r.standard_normal(L)
    return (h / np.sqrt(L)).astype(coef_dt)


def scale_of(coef_dt):
    return coef_dt(0.75 - 0.5j) if np.dtype(coef_dt).kind == "c" else coef_dt(0.75)


def white_input(n, sample_dt, seed):
    r = np.random.default_rng(seed)
    x = r.standard_normal(n)
    if np.dtype(sample_dt).kind == "c":
        x = x + 1j * r.standard_normal(n)
    return x.astype(sample_dt)


def wide(dt):
    return C128 if np.dtype(dt).kind == "c" else F64


@functools.lru_cache(maxsize=None)
def stream_of(pair, n):
    """n white samples at the pair's sample type, read-only, one stream per pair and length"""
    x = white_input(n, PAIRS[pair][2], 2000 + PAIRS[pair][0])
    x.setflags(write=False)
    return x


def inputs(pair, L, n):
    """taps, scale and n white samples at the handle's types, read-only"""
    cdt = PAIRS[pair][1]
    h = white_taps(L, cdt, 1000 + 7 * L + PAIRS[pair][0])
    h.setflags(write=False)
    return h, scale_of(cdt), stream_of(pair, n)


# ---------------------------------------------------------------- section 8d
def bound_8d(pair, h, s, x):
    return tol_of(pair) * float(np.sum(np.abs(h.astype(C128)))) * abs(complex(s)) * float(np.max(np.abs(x)))


def measure_8d(y, ref):
    y = np.asarray(y, dtype=C128)
    ref = np.asarray(ref, dtype=C128)
    assert y.shape == ref.shape, (y.shape, ref.shape)
    rr = float(np.linalg.norm(y - ref) / max(np.linalg.norm(ref), 1e-300))
    ma = float(np.max(np.abs(y - ref))) if y.size else 0.0
    return rr, ma


def check_8d(pair, y, ref, h, s, x, what):
    """both criteria: rel-RMS <= tol and max-abs <= tol * sum|h| * |scale| * max|x|; printed first"""
    rr, ma = measure_8d(y, ref)
    bound = bound_8d(pair, h, s, x)
    print(f"{what}: rel-RMS {rr:.3e} max-abs {ma:.3e} (bound {bound:.3e}, {ma / bound:.4f} of it)")
    assert rr <= tol_of(pair), (what, rr)
    assert ma <= bound, (what, ma, bound)
    return rr, ma / bound


# ---------------------------------------------------------------- the kernel's summation order
def model_f32(pair, M, K, V, h, s, x):
    """decim_poly_kernel's summation order on a fresh handle's first call, in unfused numpy f32:
    lane q adds its K * V products tap[k][e] * X[m - k][q V + e] in the walk's order (rows oldest
    first, e ascending, sdsp_decim_walk.hpp:144-151), the MV partials of an output are summed as
    the reduction does (:160-182: left to right over MV columns when CH >= MV, else P parts of CH
    columns left to right and an xor tree over the parts), then the scale (:169, :181)"""
    _, cdt, sdt, _ = PAIRS[pair]
    MV, _, CH, P, _, _ = geometry(pair, M, K, V)
    L = M * K
    j0 = M - 1
    nout = output_count(M, 0, len(x))
    # rows[rho + K - 1][c] = ext(j0 + rho M - (M - 1) + c): K - 1 rows of zero history in front
    rows = np.concatenate([np.zeros((K - 1) * M, sdt), x[:nout * M]]).reshape(nout + K - 1, M)
    cr = h[::-1]
    part = np.zeros((nout, MV), sdt)
    for k in range(K - 1, -1, -1):  # row m - k: oldest first
        X = rows[K - 1 - k:K - 1 - k + nout]
        for e in range(V):
            cols = np.arange(MV) * V + e
            tap = cr[k * M + (M - 1 - cols)].astype(cdt)
            part = (part + (tap[None, :] * X[:, cols]).astype(sdt)).astype(sdt)
    if CH >= MV:
        acc = part[:, 0]
        for c in range(1, MV):
            acc = (acc + part[:, c]).astype(sdt)
    else:
        parts = []
        for p in range(P):
            a = part[:, p * CH]
            for c in range(1, CH):
                a = (a + part[:, p * CH + c]).astype(sdt)
            parts.append(a)
        while len(parts) > 1:  # lanes q ^ CH, then q ^ 2 CH
            parts = [(parts[i] + parts[i + 1]).astype(sdt) for i in range(0, len(parts), 2)]
        acc = parts[0]
    return (acc * cdt(s)).astype(sdt)


def ref_f64(h, s, x, M, ci=0):
    """y[m] = scale * sum_i h[L - 1 - i] ext(j0 + m M - i) on a zero history, in f64 / complex128
    (the reference stores the taps reversed and walks them forward, kern_decim.hip:3-4)"""
    w = wide(x.dtype)
    full = np.convolve(x.astype(w), h[::-1].astype(wide(h.dtype)))[:len(x)]
    return full[j0_of(M, ci)::M] * wide(h.dtype)(s)


# ---------------------------------------------------------------- just off the rule
OFF_RULE = [(48, 16), (16, 16), (512, 16), (100, 16), (56, 7), (256, 128), (512, 64), (128, 32)]  # (L, M)


def off_rule_cases():
    """every (pair, L, M) of OFF_RULE that the dispatch turns away for that pair"""
    return [(pair, L, M) for L, M in OFF_RULE for pair in PAIRS if not on_rule(pair, L, M)]
