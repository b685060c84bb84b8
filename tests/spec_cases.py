"""Numpy restatements for the spectrometer (sdsp_spec_*, solid_dsp_amd.Spectrometer) and the inputs its
tests share.  No GPU import: tests/test_spec_capi.py pins these functions on the CPU,
tests/test_gpu_spec.py holds the handle to them.

Per stream, Y[m] is the oversampled channeliser's frame m (tests/oschan_cases.py), p[m][k] =
Y.re Y.re + Y.im Y.im, and spectrum j integrates frames jA .. jA + A - 1 in sub-blocks of 32 frames
counted from frame jA (the last one shorter when 32 does not divide A):

    s_b[k] = ((0 + p[jA + 32 b][k]) + p[jA + 32 b + 1][k]) + ..
    P_j[k] = (((0 + s_0) + s_1) + ..) * scale

- spec_fold: that order in the handle's real type T, one rounded operation per numpy op, with the state
  (filled, sub, tot) carried in and out, so a split call can be restated;
- spec_ref: the definition in complex128 / float64 on oschan_ref;
- spec_f32: what f32 arithmetic alone gives (oschan_f32 behind the f32 fold);
- spec_plan: kern_spec.hip's spec_plan restated.
"""
from __future__ import annotations

import functools

import numpy as np

from oschan_cases import (C64, C128, F32, TOL, coef_dtype, hist_len, name, oschan_f32, oschan_ref,  # noqa: F401
                          slide_fits, taps_len, white_streams, white_taps)

F64 = np.float64
TUNE_KERNEL, TUNE_SUBBLOCKS = 31, 32  # SDSP_TUNE_SPEC_KERNEL, SDSP_TUNE_SPEC_SUBBLOCKS
SUB = 32           # frames of a whole sub-block
MAX_A = 32768
FRAMES = 230
# one frame; calls that close no sub-block; 34 closes a sub-block and (at A > 45) no integration; the
# cuts fall on 31, 32 and 33 frames; 89 frames close several integrations at A = 5
BLOCKS = [1, 2, 8, 34, 31, 32, 33, 89]
S3 = 3
AS = (1, 5, 31, 32, 33, 64, 65, 100)


def power(Y, T):
    """p = re re + im im in T: two rounded products and one rounded sum"""
    Y = np.asarray(Y)
    if not np.iscomplexobj(Y):
        assert Y.dtype == T
        return Y
    re, im = np.ascontiguousarray(Y.real), np.ascontiguousarray(Y.imag)
    assert re.dtype == T, (re.dtype, T)
    p = re * re + im * im
    assert p.dtype == T
    return p


def spec_fold(Y_or_p, A, filled, sub, tot, scale, T, cut=SUB, restart=True, flat=False, m0=0):
    """Frames [..., frames, M] (complex frames Y of the handle's sample type, or their powers p in T)
    through the two-level sum, starting `filled` frames into an integration with the open sub-block's
    sum `sub` and the closed sub-blocks' sum `tot` ([..., M] in T, zeros when None).  Returns
    (spectra [..., J, M], filled, sub, tot).

    The mistakes test_what_the_inputs_see looks for: `cut` frames per sub-block instead of 32;
    restart=False cuts where the stream's frame index (m0 + f) is a multiple of 32, not where the
    integration's is; flat=True adds every frame straight onto `tot` (the other nesting)."""
    p = power(Y_or_p, T)
    lead, M = p.shape[:-2], p.shape[-1]
    sub = np.zeros(lead + (M,), T) if sub is None else np.array(sub, dtype=T)
    tot = np.zeros(lead + (M,), T) if tot is None else np.array(tot, dtype=T)
    scale = T(scale)
    out = []
    for f in range(p.shape[-2]):
        pf = p[..., f, :]
        if flat:
            tot = tot + pf
        else:
            sub = sub + pf
        filled += 1
        at_cut = filled % cut == 0 if restart else (m0 + f + 1) % cut == 0
        if (at_cut or filled == A) and not flat:
            tot = tot + sub
            sub = np.zeros_like(sub)
        if filled == A:
            out.append(tot * scale)
            tot = np.zeros_like(tot)
            filled = 0
    assert sub.dtype == T and tot.dtype == T
    spectra = np.stack(out, axis=-2) if out else np.zeros(lead + (0, M), T)
    assert spectra.dtype == T
    return spectra, filled, sub, tot


def spec_ref(h, M, D, A, x, prec=C64, scale=1.0):
    """the definition in complex128 / float64: [J, M], J = frames // A"""
    Y = oschan_ref(h, M, D, x, prec)
    J = len(Y) // A
    p = Y.real ** 2 + Y.imag ** 2
    return p[:J * A].reshape(J, A, M).sum(axis=1) * float(scale)


def spec_f32(h, M, D, A, x):
    """oschan_f32 behind the f32 fold: [J, M] float32"""
    return spec_fold(oschan_f32(h, M, D, x), A, 0, None, None, 1.0, F32)[0]


def count(D, A, filled, n):
    """sdsp_spec_count by a frame walk"""
    spectra = 0
    for _ in range(n // D):
        filled += 1
        if filled == A:
            spectra, filled = spectra + 1, 0
    return spectra, filled


def spec_plan(M, K, D, A, prec, kernel=0, subblocks=0):
    """kern_spec.hip spec_plan: (kernel, sub-blocks per workgroup).
    kernel (its lines `fits`, `pays`, `p.kernel`): a sliding request runs where the ring (K M + D
    samples) and the Stockham pair (2 M) fit 128 KiB; automatic is the sliding kernel where ring, pair
    and twiddle table take at most 40 KiB, but for K = 1 at M = 256 (measured).
    sub-blocks (its lines `p.subblocks`): the knob when set; automatic is 1 on the per-frame kernel and,
    on the sliding kernel, the smallest count whose frames (min(A, 32) each) reach
    4 ceil((K M - D) / D), at least 1."""
    size = np.dtype(prec).itemsize
    fits = (K * M + D + 2 * M) * size <= 128 * 1024
    pays = (K * M + D + 3 * M) * size <= 40 * 1024 and not (K == 1 and M == 256)
    k = 2 if (kernel == 2 and fits) or (kernel == 0 and pays) else 1
    if subblocks > 0:
        return k, subblocks
    if k == 1:
        return k, 1
    fill, per = -(-hist_len(M, K, D) // D), min(A, SUB)
    return k, max(1, -(-4 * fill // per))


# ---------------------------------------------------------------- the case tables
def _shapes():
    """(M, K, D, A, prec): every K with every M, every frame-stride class (1, M/2, 3M/4, M, a non-divisor)
    with every M, as test_gpu_oschan._triples spreads them; the eight integrations walk along, so that
    every A meets both kernels and both precisions (test_the_grid_covers_every_class)"""
    Ks, out, seen = (1, 3, 8, 12), [], set()
    for pi, prec in enumerate((C64, C128)):
        i = 3 * pi
        for a, (M, odd) in enumerate(((4, 3), (64, 37), (256, 201), (1024, 1000), (4096, 4001))):
            Ds = (1, M // 2, 3 * M // 4, M, odd)
            for b in range(5):
                K, D = Ks[(a + b) % 4], Ds[b]
                if (M, K, D, prec) in seen:
                    continue
                seen.add((M, K, D, prec))
                out.append((M, K, D, AS[i % 8], prec))
                i += 3  # (3 and 8 are coprime: the walk visits every A)
    return out


SHAPES = _shapes()
SHAPE_IDS = [f"{M}-{K}-{D}-A{A}-{name(p)}" for M, K, D, A, p in SHAPES]
SETTINGS = [(1, 0), (1, 3), (2, 0), (2, 1), (2, 3)]  # (kernel knob, sub-blocks knob)
# the definition test: both kernels, both precisions, A below, at and above a sub-block
DEFINITION = [(64, 8, 48, 100, C64), (64, 3, 64, 5, C128), (256, 1, 128, 33, C64), (1024, 3, 1000, 32, C64),
              (1024, 12, 512, 65, C128), (4096, 1, 4096, 31, C64)]


@functools.lru_cache(maxsize=None)
def white_input(M, K, D, prec=C64, frames=FRAMES, S=S3):
    """(taps, [S, frames D] streams)"""
    return white_taps(taps_len(M, K), prec), white_streams(S, frames * D, prec)
