"""The oversampled channeliser (solid_dsp_amd.OversampledChannelizer, sdsp_oschan_*) on the device: both
kernels at every channel count's workgroup shape, branch depth and frame-stride class, against the
complex128 definition, against each other bit for bit, against the rotated sums done in numpy in front of
an FFT handle bit for bit, against sd.Channelizer at D = M and against the down-converter form.

Inputs (tests/oschan_cases.py; tests/test_oschan_capi.py shows on the CPU what they can see): white taps,
white streams from O.synth, three streams, 45 frames fed in calls of 1, 2, 8 and 34 frames through
execute_block_device: one frame, a call shorter than the history, and odd frame counts at every cut, so
that frames D mod M != 0 there for every D but M.  Tolerance, per stream (section 8d): tol = 1e-6 for
complex64, 1e-12 for complex128, on
    rel_rms(y, ref) <= tol   and   for every frame m  ||y[m] - ref[m]|| <= tol sqrt(mean_m ||ref[m]||^2)
test_f32_arithmetic_alone_stays_inside (test_oschan_capi.py) shows f32 arithmetic alone below half of both.
"""
import functools

import numpy as np
import pytest

from gpu_util import bits_equal, empty_dev, rel_rms, to_dev, to_host
from oschan_cases import (AMP, BLOCKS, auto_frames, auto_slides, C64, C128, FRAMES, TOL, TUNE_FPB, TUNE_KERNEL, check_streams, ddc_form,
                          hist_len, name, oschan_exact, slide_fits, taps_len, white_case, white_streams, white_taps)

gpu = pytest.mark.gpu

sd = pytest.importorskip("solid_dsp_amd")

E_INVALID_ARGUMENT = 90
S3 = 3  # streams of every white case


# ---------------------------------------------------------------- helpers
def offset_view(count, prec, off):
    """a device buffer of `count` samples whose address is `off` samples past an allocation"""
    return empty_dev(count + off, prec)[off:]


def run_blocks(ch, x, blocks, in_off=0, out_off=0):
    """feed [S, frames D] through execute_block_device in calls of blocks[i] frames on the current
    stream, every output buffer filled with NaN first; the phase is checked after each call.
    [S, frames, M]"""
    import torch
    S, M, D = x.shape[0], ch.M, ch.D
    prec = x.dtype.type
    assert sum(blocks) * D == x.shape[1]
    st = torch.cuda.current_stream()
    y = np.zeros((S, sum(blocks), M), prec)
    a = 0
    for nb in blocks:
        b = a + nb
        d_in = offset_view(S * nb * D, prec, in_off)
        d_in.copy_(to_dev(np.ascontiguousarray(x[:, a * D:b * D]).reshape(-1)))
        d_out = offset_view(S * nb * M, prec, out_off)
        d_out.fill_(complex(float("nan"), float("nan")))
        if prec == C64:
            assert d_in.data_ptr() % 16 == 8 * in_off and d_out.data_ptr() % 16 == 8 * out_off
        assert ch.execute_block_device(d_in, nb * D, d_out, st) == nb
        assert ch.phase == (b * D) % M, f"phase {ch.phase} after {b} frames, the host counts {(b * D) % M}"
        y[:, a:b] = to_host(d_out).reshape(S, nb, M)
        a = b
    return y


def tuned(h, M, D, S, prec=C64, kernel=None, fpb=None):
    ch = sd.OversampledChannelizer(h, M, D, sample_dtype=prec, streams=S)
    for key, v in ((TUNE_KERNEL, kernel), (TUNE_FPB, fpb)):
        if v is not None:
            ch.set_tuning(key, v)
    return ch


@functools.lru_cache(maxsize=None)
def run_case(M, K, D, prec, kernel, fpb):
    """the white case of one shape on one kernel setting, run once and shared; [3, 45, M]"""
    h, x, _ = white_case(M, K, D, S3, FRAMES, prec)
    ch = tuned(h, M, D, S3, prec, kernel, fpb)
    assert (ch.M, ch.D, ch.K, ch.phase) == (M, D, K, 0)
    k, f = ch.info()
    want = 2 if kernel == 2 and slide_fits(M, K, D, prec) else 1
    assert k == want, f"info() reports kernel {k}, the shape and the knob give {want}"
    if k == 1:
        assert f == 1
    elif fpb:
        assert f == fpb
    else:
        assert f == auto_frames(M, K, D)  # automatic: the fill stays below the chunk's own reads
    y = run_blocks(ch, x, BLOCKS)
    y.setflags(write=False)
    return y


def flat(y):
    return y.reshape(len(y), -1)


def _triples():
    """eight (M, K, D) per channel count: every K with every M, every frame-stride class (1, M/2, 3M/4,
    M, a non-divisor) with every M, and every K with every class somewhere"""
    Ks, out = (1, 3, 8, 12), []
    for a, (M, odd) in enumerate(((4, 3), (8, 5), (64, 37), (1024, 1000), (4096, 4001))):
        Ds = (1, M // 2, 3 * M // 4, M, odd)
        out += [(M, Ks[(a + b) % 4], Ds[b]) for b in range(5)]
        out += [(M, Ks[(a + b + 2) % 4], Ds[b]) for b in (1, 2, 4)]
    return list(dict.fromkeys(out))  # (at M = 4 the non-divisor 3 is 3M/4 too: two triples fewer)


TRIPLES = _triples()
SHAPES = [(M, K, D, prec) for prec in (C64, C128) for M, K, D in TRIPLES]
SHAPE_IDS = [f"{M}-{K}-{D}-{name(p)}" for M, K, D, p in SHAPES]
SETTINGS = [(1, 0), (2, 1), (2, 3), (2, 128)]


def test_the_grid_covers_every_class():
    assert len(TRIPLES) == 38
    for M in (4, 8, 64, 1024, 4096):
        mine = [(K, D) for m, K, D in TRIPLES if m == M]
        assert {K for K, _ in mine} == {1, 3, 8, 12}
        assert {1, M // 2, 3 * M // 4, M} <= {D for _, D in mine}
        assert any(M % D for _, D in mine)


# ================================================================ A. tolerance, every shape and setting
@gpu
@pytest.mark.parametrize("kernel,fpb", SETTINGS, ids=[f"k{k}-f{f}" for k, f in SETTINGS])
@pytest.mark.parametrize("M,K,D,prec", SHAPES, ids=SHAPE_IDS)
def test_every_shape_and_setting(M, K, D, prec, kernel, fpb):
    """both kernels at every workgroup shape of the launcher, K = 1, 3 (with a tap tail that must be
    ignored), 8 (the deepest register instance) and 12 (coefficients re-read); frames per block of 1
    and 3 put chunk boundaries inside every call, 128 makes one chunk of each call"""
    _, _, ref = white_case(M, K, D, S3, FRAMES, prec)
    check_streams(flat(run_case(M, K, D, prec, kernel, fpb)), flat(ref), M, TOL[prec],
                  f"A M={M} K={K} D={D} {name(prec)} kernel={kernel} fpb={fpb}")


# ================================================================ B. the kernels agree bit for bit
@gpu
@pytest.mark.parametrize("M,K,D,prec", SHAPES, ids=SHAPE_IDS)
def test_kernels_bit_identical(M, K, D, prec):
    """across kernels and frames per block; and one call of 45 frames gives the bits of the four calls"""
    base = run_case(M, K, D, prec, 1, 0)
    assert not np.isnan(base).any()
    for kernel, fpb in SETTINGS:
        assert bits_equal(run_case(M, K, D, prec, kernel, fpb), base), \
            f"M={M} K={K} D={D} {name(prec)}: kernel {kernel} at {fpb} frames per block differs from the per-frame kernel"
    h, x, _ = white_case(M, K, D, S3, FRAMES, prec)
    for kernel, fpb in ((1, 0), (2, 3)):
        whole = run_blocks(tuned(h, M, D, S3, prec, kernel, fpb), x, [FRAMES])
        assert bits_equal(whole, base), f"M={M} K={K} D={D} {name(prec)} kernel {kernel}: one call differs from four"


# ================================================================ C. bit-identity with the FFT handle
@gpu
@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("prec", [C64, C128], ids=["c64", "c128"])
@pytest.mark.parametrize("K", [1, 5])
@pytest.mark.parametrize("M,D", [(8, 1), (8, 6), (8, 8), (64, 1), (64, 48), (64, 64), (1024, 1), (1024, 768),
                                 (1024, 1024)])
def test_bit_identical_to_sums_on_the_fft_handle(M, D, K, prec, kernel):
    """sd.FFT(M, FORWARD) on oschan_exact's rotated sums of the same stream, the zero history included,
    equals the handle's output bit for bit"""
    h, x, _ = white_case(M, K, D, S3, FRAMES, prec)
    fft = sd.FFT(M, sd.FFTDirection.FORWARD, precision=prec)
    y = run_case(M, K, D, prec, kernel, 0)
    for s in range(S3):
        w = oschan_exact(h, M, D, np.concatenate([np.zeros(hist_len(M, K, D), prec), x[s]]), 0, prec)
        Y = fft.execute(np.ascontiguousarray(w))
        assert Y.dtype == prec and Y.shape == (FRAMES, M)
        assert bits_equal(y[s], Y), f"M={M} K={K} D={D} {name(prec)} kernel={kernel} stream {s}"


# ================================================================ D. D = M is the channeliser
@gpu
@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("M,K,prec", [(4, 3, C64), (64, 8, C64), (4096, 1, C64), (1024, 3, C64), (64, 8, C128),
                                      (1024, 3, C128)],
                         ids=["4-3-c64", "64-8-c64", "4096-1-c64", "1024-3-c64", "64-8-c128", "1024-3-c128"])
def test_critically_sampled_is_the_channelizer(M, K, prec, kernel):
    """D = M against sd.Channelizer on the same calls: bit-identical wherever that runs chan_kernel
    (complex128, and every complex64 M but 1024); within tol at M = 1024 in complex64, where it runs its
    streaming kernel"""
    import torch
    h, x, _ = white_case(M, K, M, S3, FRAMES, prec)
    cz = sd.Channelizer(h, M, sample_dtype=prec, streams=S3)
    st = torch.cuda.current_stream()
    z = np.zeros((S3, FRAMES, M), prec)
    a = 0
    for nb in BLOCKS:
        d_out = empty_dev(S3 * nb * M, prec)
        cz.execute_block_device(to_dev(np.ascontiguousarray(x[:, a * M:(a + nb) * M]).reshape(-1)), nb * M, d_out, st)
        z[:, a:a + nb] = to_host(d_out).reshape(S3, nb, M)
        a += nb
    y = run_case(M, K, M, prec, kernel, 0)
    if prec == C64 and M == 1024:
        check_streams(flat(y), flat(z.astype(C128)), M, TOL[prec], f"D M={M} K={K} against the streaming channeliser")
    else:
        assert bits_equal(y, z), f"M={M} K={K} {name(prec)} kernel={kernel}"


# ================================================================ E. every channel is a down-converter
@functools.lru_cache(maxsize=None)
def ddc_ref(M, K, D):
    h, x, _ = white_case(M, K, D, S3, FRAMES, C64)
    return ddc_form(h, M, D, x[1])


@gpu
@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("M,K,D", [(64, 8, 48), (1024, 3, 1000)])
def test_channels_match_the_down_converter_form(M, K, D, kernel):
    """each channel of a device run against ddc_form (mix, convolve, decimate), within tol of the
    channel's own norm"""
    y = run_case(M, K, D, C64, kernel, 0)
    ref = ddc_ref(M, K, D)
    worst = max(rel_rms(y[1][:, k], ref[:, k]) for k in range(M))
    print(f"E ddc form M={M} K={K} D={D} kernel={kernel}: worst channel rel-RMS {worst:.3e} (limit 1e-06)")
    assert worst <= TOL[C64]


# ================================================================ F. impulses
BLOCKS_F = [20, 25]
FPB_F = 8  # sliding kernel: chunk boundaries at frames 8, 16 (and 24) of a call


@gpu
@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("M,K,D,prec", [(16, 3, 12, C64), (64, 5, 37, C128), (1024, 3, 512, C64)],
                         ids=["16-3-12-c64", "64-5-37-c128", "1024-3-512-c64"])
def test_impulses(M, K, D, prec, kernel):
    """single samples x[n0] = AMP on the middle of three streams: the first sample, one whose response
    straddles the call boundary (it arrives through the history) and one whose response straddles a
    chunk boundary of the second call (through the chunk's fill).  By the down-converter form, frame m of
    that stream is AMP g[t] e^{+j 2 pi k (n0 + 1) / M} over the channels k wherever
    t = (m+1) D - 1 - n0 lies in [0, K M), each within tol of its own norm; every other output of every
    stream is exactly zero"""
    total, tol, s0 = sum(BLOCKS_F), TOL[prec], 1
    what = f"F impulses M={M} K={K} D={D} {name(prec)} kernel={kernel}"
    h = white_taps(M * K, prec)
    g = np.asarray(h).astype(np.float64).reshape(K, M)[::-1].reshape(-1)  # g[p + i M] = h[p + (K-1-i) M]
    sites = [0, BLOCKS_F[0] * D - 2, (BLOCKS_F[0] + 2 * FPB_F) * D - 1 - M // 2]
    assert all(b - a >= K * M + D for a, b in zip(sites[:-1], sites[1:])), sites  # responses do not meet
    x = np.zeros((S3, total * D), prec)
    expect = {}
    k = np.arange(M)
    for n0, cut in zip(sites, (None, BLOCKS_F[0], BLOCKS_F[0] + 2 * FPB_F)):
        x[s0, n0] = AMP
        hit = [m for m in range(total) if 0 <= (m + 1) * D - 1 - n0 < K * M]
        assert cut is None or hit[0] < cut <= hit[-1], (n0, hit)  # the response straddles the boundary
        for m in hit:
            assert m not in expect
            expect[m] = AMP * g[(m + 1) * D - 1 - n0] * np.exp(2j * np.pi * ((k * (n0 + 1)) % M) / M)
    y = run_blocks(tuned(h, M, D, S3, prec, kernel, FPB_F), x, BLOCKS_F)
    silent = np.ones((S3, total), bool)
    silent[s0, list(expect)] = False
    stray = int(np.count_nonzero(y[silent]))
    worst = 0.0
    for m, e in sorted(expect.items()):
        rel = rel_rms(y[s0, m], e)
        worst = max(worst, rel)
        assert rel <= tol, f"{what}: response frame {m} rel-RMS {rel:.3e} > {tol:.0e}"
    print(f"{what}: {len(expect)} response frames, worst rel-RMS {worst:.3e} (limit {tol:.0e}); "
          f"{stray} non-zero outputs among {int(silent.sum())} silent frames")
    assert stray == 0, f"{what}: {stray} non-zero outputs outside the responses"


# ================================================================ G. which kernel runs
LIMITS = [  # (M, the largest K whose ring and pair fit 128 KiB at every D, prec); 0: no K fits
    (1024, 13, C64), (1024, 5, C128), (4096, 1, C64), (4096, 0, C128)]


@gpu
@pytest.mark.parametrize("M,K,prec", LIMITS, ids=[f"{M}-{K}-{name(p)}" for M, K, p in LIMITS])
def test_sliding_kernel_at_its_limits(M, K, prec):
    """the largest K that fits (at D = M: 128 KiB to the byte at M = 1024, K = 13 and at M = 4096, K = 1
    in complex64, where the twiddle table fills the LDS to 160 KiB) runs the sliding kernel; the first K
    that does not fit reports the per-frame kernel for a sliding request and gives the same results.
    No K fits at M = 4096 in complex128"""
    for D in (M, 3 * M // 4):
        if K:
            assert slide_fits(M, K, D, prec)
            _, _, ref = white_case(M, K, D, S3, FRAMES, prec)
            base = run_case(M, K, D, prec, 1, 0)
            check_streams(flat(base), flat(ref), M, TOL[prec], f"G M={M} K={K} D={D} {name(prec)} kernel=1")
            for fpb in (3, 128):
                assert bits_equal(run_case(M, K, D, prec, 2, fpb), base), f"sliding kernel at {fpb} frames per block"
        assert not slide_fits(M, K + 1, D, prec)
        h = white_taps(taps_len(M, K + 1), prec)
        assert tuned(h, M, D, S3, prec, kernel=2).info() == (1, 1)
        _, _, ref = white_case(M, K + 1, D, S3, FRAMES, prec)
        y = run_case(M, K + 1, D, prec, 2, 0)
        check_streams(flat(y), flat(ref), M, TOL[prec], f"G fallback M={M} K={K + 1} D={D} {name(prec)}")
        assert bits_equal(y, run_case(M, K + 1, D, prec, 1, 0))


@gpu
def test_automatic_choice_is_the_sliding_kernel_where_the_plan_says():
    """automatic: the sliding kernel where oschan_plan's measured rule puts it (a footprint of at most
    16 KiB), at its automatic frames per workgroup; a sliding request runs wherever the kernel fits"""
    both = set()
    for M, K, D, prec in SHAPES + [(128, 8, 64, C64), (128, 12, 64, C64), (256, 8, 128, C64), (128, 8, 64, C128)]:
        ch = sd.OversampledChannelizer(white_taps(taps_len(M, K), prec), M, D, sample_dtype=prec)
        want = (2, auto_frames(M, K, D)) if auto_slides(M, K, D, prec) else (1, 1)
        assert ch.info() == want, (M, K, D, name(prec))
        ch.set_tuning(TUNE_KERNEL, 2)
        assert ch.info()[0] == (2 if slide_fits(M, K, D, prec) else 1), (M, K, D, name(prec))
        both.add(want[0])
    assert both == {1, 2}
    assert auto_slides(128, 12, 64, C64) and not auto_slides(256, 8, 128, C64) and not auto_slides(128, 8, 64, C128)
    ch = sd.OversampledChannelizer(white_taps(1024 * 5), 1024, 768)
    assert ch.info() == (1, 1)  # automatic at 1024 channels: the per-frame kernel
    ch.set_tuning(TUNE_KERNEL, 2)
    assert ch.info() == (2, auto_frames(1024, 5, 768))
    ch.set_tuning(TUNE_KERNEL, 1)
    assert ch.info() == (1, 1)
    ch.set_tuning(TUNE_KERNEL, 2)
    ch.set_tuning(TUNE_FPB, 7)
    assert ch.info() == (2, 7)
    for key, v in ((TUNE_KERNEL, 3), (TUNE_KERNEL, -1), (TUNE_FPB, -1), (25, 1)):
        with pytest.raises(sd.SdspError) as e:
            ch.set_tuning(key, v)
        assert e.value.code == E_INVALID_ARGUMENT


# ================================================================ H. the boundary
@gpu
@pytest.mark.parametrize("kernel", [1, 2])
def test_host_blocks_two_streams(kernel):
    """execute_block with a host [2, n] array per call (the staged path), M = 128, K = 5, D = 96; and a
    single-stream handle takes [n]"""
    M, K, D, S = 128, 5, 96, 2
    h, x, ref = white_case(M, K, D, S)
    ch = tuned(h, M, D, S, C64, kernel, 3)
    cuts = np.cumsum([0] + BLOCKS) * D
    y = np.concatenate([ch.execute_block(x[:, a:b]) for a, b in zip(cuts[:-1], cuts[1:])], axis=1)
    assert y.shape == (S, FRAMES, M)
    check_streams(flat(y), flat(ref), M, 1e-6, f"H host blocks M={M} K={K} D={D} S={S} kernel={kernel}")
    one = tuned(h, M, D, 1, C64, kernel, 3)
    y0 = np.concatenate([one.execute_block(x[0, a:b]) for a, b in zip(cuts[:-1], cuts[1:])])
    assert y0.shape == (FRAMES, M) and bits_equal(y0, y[0])


@gpu
@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("M,K,D", [(64, 8, 37), (1024, 3, 768)])
def test_8_byte_aligned_blocks(M, K, D, kernel):
    """input and output each one complex64 past a 16-byte boundary: the same bits as aligned blocks"""
    h, x, ref = white_case(M, K, D, S3)
    y = run_blocks(tuned(h, M, D, S3, C64, kernel, 3), x, BLOCKS, in_off=1, out_off=1)
    check_streams(flat(y), flat(ref), M, 1e-6, f"H 8-byte aligned M={M} K={K} D={D} kernel={kernel}")
    assert bits_equal(y, run_case(M, K, D, C64, kernel, 3))


@gpu
@pytest.mark.parametrize("kernel", [1, 2])
def test_refused_calls_leave_history_and_phase_untouched(kernel):
    """n % D != 0 and overlapping input and output are refused with SDSP_E_INVALID_ARGUMENT; the phase
    stays, and the next valid call equals an undisturbed handle's, bit for bit.  n = 0 returns 0 frames
    and changes nothing"""
    import torch
    M, K, D, S = 64, 4, 48, 2
    h = white_taps(M * K)
    x = white_streams(S, 9 * D)
    st = torch.cuda.current_stream()

    def call(ch, a, b):
        d_in = to_dev(np.ascontiguousarray(x[:, a * D:b * D]).reshape(-1))
        d_out = empty_dev(S * (b - a) * M, C64)
        assert ch.execute_block_device(d_in, (b - a) * D, d_out, st) == b - a
        return to_host(d_out)

    calm, poked = tuned(h, M, D, S, C64, kernel, 2), tuned(h, M, D, S, C64, kernel, 2)
    assert bits_equal(call(calm, 0, 3), call(poked, 0, 3))
    phase = (3 * D) % M
    assert phase != 0 and poked.phase == phase
    d_in, d_out = to_dev(np.ascontiguousarray(x[:, 3 * D:9 * D]).reshape(-1)), empty_dev(S * 6 * M, C64)
    for n in (D + 1, D - 1, 5 * D - 3):
        with pytest.raises(sd.SdspError) as e:
            poked.execute_block_device(d_in, n, d_out, st)
        assert e.value.code == E_INVALID_ARGUMENT and "whole number" in str(e.value)
        assert poked.phase == phase
    for out in (d_in, d_in[D:]):  # the same block; a block that starts inside the input
        with pytest.raises(sd.SdspError) as e:
            poked.execute_block_device(d_in, 2 * D, out, st)
        assert e.value.code == E_INVALID_ARGUMENT and "overlap" in str(e.value)
        assert poked.phase == phase
    # the host entry point refuses a ragged n before it reads the block
    assert sd.lib().sdsp_oschan_execute_block(poked._h, None, D + 1, None, None) == E_INVALID_ARGUMENT
    assert poked.execute_block_device(d_in, 0, d_out, st) == 0
    assert poked.phase == phase
    assert bits_equal(call(calm, 3, 9), call(poked, 3, 9))
    assert poked.phase == (9 * D) % M


@gpu
@pytest.mark.parametrize("kernel", [1, 2])
def test_reset_and_set_streams_zero_history_and_phase(kernel):
    M, K, D, S = 64, 4, 48, 2
    h = white_taps(M * K)
    x = white_streams(S, 6 * D)
    fresh = tuned(h, M, D, S, C64, kernel, 2).execute_block(x[:, 3 * D:])
    assert not bits_equal(fresh, tuned(h, M, D, S, C64, kernel, 2).execute_block(x)[:, 3:])  # the state matters
    ch = tuned(h, M, D, S, C64, kernel, 2)
    ch.execute_block(x[:, :3 * D])
    assert ch.phase == (3 * D) % M != 0
    ch.reset()
    assert ch.phase == 0
    assert bits_equal(ch.execute_block(x[:, 3 * D:]), fresh)
    ch.set_streams(1)
    assert ch.phase == 0
    ch.execute_block(x[0, :3 * D])
    assert ch.phase != 0
    ch.set_streams(S)
    assert ch.phase == 0
    assert bits_equal(ch.execute_block(x[:, 3 * D:]), fresh)
