"""The synthesis channeliser (solid_dsp_amd.ChannelSynthesizer, sdsp_ichan_*) on the device: both kernels
at every channel count's workgroup shape, against the complex128 definition, against each other bit for
bit, and against the same sums done in numpy on the output of an FFT handle, bit for bit.

Inputs (tests/ichan_cases.py; tests/test_ichan_capi.py shows on the CPU what they can see): white taps,
white channel samples from O.synth, three streams, calls of 1, K + 2, 2 and 4 frames through
execute_block_device; impulses, whose response is known in closed form and outside of which every output
is exactly zero.  Tolerance, per stream (section 8d): tol = 1e-6 for complex64, 1e-12 for complex128, on
    rel_rms(y, ref) <= tol   and   for every frame m  ||y[m] - ref[m]|| <= tol sqrt(mean_m ||ref[m]||^2)
test_f32_arithmetic_alone_stays_inside (test_ichan_capi.py) shows f32 arithmetic alone below half of both.
"""
import functools

import numpy as np
import pytest

import oracle_lib as O
from gpu_util import bits_equal, empty_dev, rel_rms, to_dev, to_host
from ichan_cases import (AMP, C64, C128, TOL, TUNE_FPB, TUNE_KERNEL, blocks_a, check_streams, ichan_exact,
                         ichan_ref, name, pair_identity, taps_len, white_case, white_frames, white_taps)

gpu = pytest.mark.gpu

sd = pytest.importorskip("solid_dsp_amd")

E_INVALID_ARGUMENT = 90
S3 = 3  # streams of every white case


# ---------------------------------------------------------------- helpers
def offset_view(count, prec, off):
    """a device buffer of `count` samples whose address is `off` samples past an allocation"""
    return empty_dev(count + off, prec)[off:]


def run_blocks(sy, X, blocks, in_off=0, out_off=0):
    """feed [S, frames, M] through execute_block_device in calls of blocks[i] frames on the current
    stream, every output buffer filled with NaN first; [S, frames M]"""
    import torch
    S, _, M = X.shape
    prec = X.dtype.type
    assert sum(blocks) == X.shape[1]
    st = torch.cuda.current_stream()
    y = np.zeros((S, sum(blocks) * M), prec)
    a = 0
    for nb in blocks:
        b = a + nb
        d_in = offset_view(S * nb * M, prec, in_off)
        d_in.copy_(to_dev(np.ascontiguousarray(X[:, a:b]).reshape(-1)))
        d_out = offset_view(S * nb * M, prec, out_off)
        d_out.fill_(complex(float("nan"), float("nan")))
        if prec == C64:
            assert d_in.data_ptr() % 16 == 8 * in_off and d_out.data_ptr() % 16 == 8 * out_off
        assert sy.execute_block_device(d_in, nb * M, d_out, st) == nb
        y[:, a * M:b * M] = to_host(d_out).reshape(S, nb * M)
        a = b
    return y


def tuned(g, M, S, prec=C64, kernel=None, fpb=None):
    sy = sd.ChannelSynthesizer(g, M, sample_dtype=prec, streams=S)
    for key, v in ((TUNE_KERNEL, kernel), (TUNE_FPB, fpb)):
        if v is not None:
            sy.set_tuning(key, v)
    return sy


def ring_fits(M, K, prec):
    return (K + 1) * M * np.dtype(prec).itemsize <= 128 * 1024


@functools.lru_cache(maxsize=None)
def run_case(M, K, prec, kernel, fpb):
    """the white case of one shape on one kernel setting, run once and shared; [3, frames M]"""
    blocks = blocks_a(K)
    g, X, _ = white_case(M, taps_len(M, K), S3, sum(blocks), prec)
    sy = tuned(g, M, S3, prec, kernel, fpb)
    assert sy.subfilter_len() == K
    k, f = sy.info()
    want = 2 if kernel == 2 and ring_fits(M, K, prec) else 1
    assert k == want, f"info() reports kernel {k}, the shape and the knob give {want}"
    if k == 1:
        assert f == 1
    elif fpb:
        assert f == fpb
    else:
        assert f >= max(8 * (K - 1), 1)  # automatic: the warm-up re-reads at most an eighth of the input
    y = run_blocks(sy, X, blocks)
    y.setflags(write=False)
    return y


SHAPES = [(M, K, prec) for prec in (C64, C128) for M in (4, 8, 32, 256, 1024, 4096) for K in (1, 2, 5)]
SHAPE_IDS = [f"{M}-{K}-{name(p)}" for M, K, p in SHAPES]
SETTINGS = [(kernel, fpb) for kernel in (1, 2) for fpb in (1, 3, 0)]


# ================================================================ A. tolerance, every shape and setting
@gpu
@pytest.mark.parametrize("kernel,fpb", SETTINGS, ids=[f"k{k}-f{f}" for k, f in SETTINGS])
@pytest.mark.parametrize("M,K,prec", SHAPES, ids=SHAPE_IDS)
def test_every_shape_and_setting(M, K, prec, kernel, fpb):
    """both kernels at every workgroup shape of the launcher (M = 8 and 32 take the radix-2 first pass,
    M = 4 is a single radix-4 pass), K = 1 (no history), 2 and 5 (with a tap tail that must be ignored);
    frames per block of 1 and 3 put chunk boundaries, and warm-ups longer than a chunk, inside every
    call"""
    _, _, ref = white_case(M, taps_len(M, K), S3, sum(blocks_a(K)), prec)
    check_streams(run_case(M, K, prec, kernel, fpb), ref, M, TOL[prec],
                  f"A M={M} K={K} {name(prec)} kernel={kernel} fpb={fpb}")


# ================================================================ B. the kernels agree bit for bit
@gpu
@pytest.mark.parametrize("M,K,prec", SHAPES, ids=SHAPE_IDS)
def test_kernels_bit_identical(M, K, prec):
    base = run_case(M, K, prec, 1, 0)
    assert not np.isnan(base).any()
    for kernel, fpb in SETTINGS:
        assert bits_equal(run_case(M, K, prec, kernel, fpb), base), \
            f"M={M} K={K} {name(prec)}: kernel {kernel} at {fpb} frames per block differs from the per-frame kernel"


@gpu
@pytest.mark.parametrize("M,K,prec", [(32, 9, C64), (32, 9, C128), (1024, 12, C64), (4096, 3, C64), (1024, 7, C128)],
                         ids=["32-9-c64", "32-9-c128", "1024-12-c64", "4096-3-c64", "1024-7-c128"])
def test_ring_kernel_at_its_limits(M, K, prec):
    """K > 8: the ring kernel has no instance with the coefficients in registers and re-reads them every
    frame.  M = 4096, K = 3 in complex64 and M = 1024, K = 7 in complex128: the largest rings (128 KiB),
    the first with its twiddle table filling the LDS to 160 KiB.  (M = 4096, K = 1 in complex128, where
    the table does not fit and stays in global memory, is among the shapes above.)  Tolerance on both
    kernels, and the same bits"""
    assert ring_fits(M, K, prec)
    _, _, ref = white_case(M, taps_len(M, K), S3, sum(blocks_a(K)), prec)
    base = run_case(M, K, prec, 1, 0)
    check_streams(base, ref, M, TOL[prec], f"B M={M} K={K} {name(prec)} kernel=1")
    for fpb in (1, 3, 0):
        y = run_case(M, K, prec, 2, fpb)
        check_streams(y, ref, M, TOL[prec], f"B M={M} K={K} {name(prec)} kernel=2 fpb={fpb}")
        assert bits_equal(y, base), f"ring kernel at {fpb} frames per block differs from the per-frame kernel"


# ================================================================ C. bit-identity with the FFT handle
@gpu
@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("prec", [C64, C128], ids=["c64", "c128"])
@pytest.mark.parametrize("K", [1, 5])
@pytest.mark.parametrize("M", [8, 64, 1024])
def test_bit_identical_to_sums_on_the_fft_handle(M, K, prec, kernel):
    """ichan_exact on sd.FFT(M, REVERSE)'s output of the same frames, the K-1 zero history frames
    included, equals the handle's output bit for bit"""
    frames = sum(blocks_a(K))
    g, X, _ = white_case(M, taps_len(M, K), S3, frames, prec)
    fft = sd.FFT(M, sd.FFTDirection.REVERSE, precision=prec)
    y = run_case(M, K, prec, kernel, 0)
    for s in range(S3):
        U = fft.execute(np.concatenate([np.zeros((K - 1, M), prec), X[s]]))
        assert U.dtype == prec and U.shape == (frames + K - 1, M)
        assert bits_equal(y[s], ichan_exact(g, M, U, prec)), f"M={M} K={K} {name(prec)} kernel={kernel} stream {s}"


# ================================================================ D. which kernel runs
@gpu
def test_ring_request_that_does_not_fit_runs_the_per_frame_kernel():
    """M = 4096, K = 5, complex64: six slots of 32 KiB are more than 128 KiB"""
    M, K = 4096, 5
    sy = tuned(white_taps(taps_len(M, K)), M, S3, C64, kernel=2)
    assert sy.info() == (1, 1)
    _, _, ref = white_case(M, taps_len(M, K), S3, sum(blocks_a(K)), C64)
    check_streams(run_case(M, K, C64, 2, 0), ref, M, 1e-6, "D fallback M=4096 K=5")


@gpu
def test_automatic_choice_is_the_ring_kernel_where_it_fits():
    sy = sd.ChannelSynthesizer(white_taps(taps_len(1024, 5)), 1024)
    assert sy.info()[0] == 2
    sy.set_tuning(TUNE_KERNEL, 1)
    assert sy.info() == (1, 1)
    sy.set_tuning(TUNE_KERNEL, 0)
    sy.set_tuning(TUNE_FPB, 7)
    assert sy.info() == (2, 7)
    for key, v in ((TUNE_KERNEL, 3), (TUNE_KERNEL, -1), (TUNE_FPB, -1), (24, 1)):
        with pytest.raises(sd.SdspError) as e:
            sy.set_tuning(key, v)
        assert e.value.code == E_INVALID_ARGUMENT
    assert sd.ChannelSynthesizer(white_taps(4096 * 3), 4096).info()[0] == 2   # K = 3 at 4096: 128 KiB
    assert sd.ChannelSynthesizer(white_taps(4096 * 4), 4096).info()[0] == 1


# ================================================================ E. impulses
BLOCKS_E = [20, 30]
FPB_E = 8  # ring kernel: chunk boundaries at frames 8, 16 and 24 of a call


def impulse_sites(M, K):
    """(frame, channel) of the impulses, at least K + 1 frames apart: the first frame; the frame before the
    call boundary (the response arrives through the history); the frame before the chunk boundary at
    frame 16 of the second call (through the warm-up); and max(K - 2, 1) frames before the end (the
    response is cut short)"""
    total = sum(BLOCKS_E)
    sites = [(0, 0), (10, M - 1), (BLOCKS_E[0] - 1, 5 % M), (BLOCKS_E[0] + 15, 300 % M),
             (total - max(K - 2, 1), M // 2)]
    fr = [f for f, _ in sites]
    assert all(b - a >= K + 1 for a, b in zip(fr[:-1], fr[1:])), fr
    assert fr[-1] + K > total  # cut short
    return sites


@gpu
@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("M,K,prec", [(16, 3, C64), (512, 4, C128), (1024, 5, C64)],
                         ids=["16-3-c64", "512-4-c128", "1024-5-c64"])
def test_impulses(M, K, prec, kernel):
    """single channel samples X[m0][k] = AMP on the middle of three streams: frame m0 + i, i < K, of that
    stream is AMP g[r + (K-1-i) M] exp(+2j pi k (M-1-r) / M), each within tol of its own norm; every
    other output of every stream is exactly zero"""
    total, tol, s0 = sum(BLOCKS_E), TOL[prec], 1
    what = f"E impulses M={M} K={K} {name(prec)} kernel={kernel}"
    g = white_taps(M * K, prec)
    X = np.zeros((S3, total, M), prec)
    expect = {}
    r = np.arange(M)
    for m0, k in impulse_sites(M, K):
        X[s0, m0, k] = AMP
        for i in range(K):
            if m0 + i < total:
                assert m0 + i not in expect
                expect[m0 + i] = AMP * g[r + (K - 1 - i) * M].astype(np.float64) * \
                    np.exp(2j * np.pi * ((k * (M - 1 - r)) % M) / M)
    y = run_blocks(tuned(g, M, S3, prec, kernel, FPB_E), X, BLOCKS_E).reshape(S3, total, M)
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
    if stray:
        where = sorted({(int(s), int(m)) for s, m in zip(*np.nonzero(np.any(y != 0, axis=-1) & silent))})
        raise AssertionError(f"{what}: {stray} non-zero outputs outside the responses, (stream, frame) {where[:12]}")


# ================================================================ F. analysis feeding synthesis
@gpu
@pytest.mark.parametrize("M,Kh,Kg", [(64, 5, 2), (1024, 3, 8)])
def test_round_trip_on_the_device(M, Kh, Kg):
    """Channelizer(h, M) feeding ChannelSynthesizer(g, M) on the device, ragged calls, complex64: within
    2e-6 rel-RMS (two f32 stages at the section 8d figure each) of the closed form in complex128"""
    import torch
    S, blocks = 2, [3, 21, 1, 20]
    frames = sum(blocks)
    h, g = white_taps(M * Kh), white_taps(M * Kg, seed=20261024)
    x = np.stack([O.synth(20261025, s, 0, M * frames, complex_=True) for s in range(S)]).astype(C64)
    ch = sd.Channelizer(h, M, sample_dtype=C64, streams=S)
    sy = sd.ChannelSynthesizer(g, M, sample_dtype=C64, streams=S)
    st = torch.cuda.current_stream()
    y = np.zeros((S, frames * M), C64)
    a = 0
    for nb in blocks:
        b = a + nb
        d_x = to_dev(np.ascontiguousarray(x[:, a * M:b * M]).reshape(-1))
        d_X, d_y = empty_dev(S * nb * M, C64), empty_dev(S * nb * M, C64)
        assert ch.execute_block_device(d_x, nb * M, d_X, st) == nb
        assert sy.execute_block_device(d_X, nb * M, d_y, st) == nb
        y[:, a * M:b * M] = to_host(d_y).reshape(S, nb * M)
        a = b
    for s in range(S):
        rel = rel_rms(y[s], pair_identity(g, h, M, x[s]))
        print(f"F round trip M={M} K_h={Kh} K_g={Kg} stream {s}: rel-RMS {rel:.3e} (limit 2e-06)")
        assert rel <= 2e-6


# ================================================================ G. the boundary
@gpu
@pytest.mark.parametrize("kernel", [1, 2])
def test_host_blocks_two_streams(kernel):
    """execute_block with a host [2, frames, M] array per call (the staged path), M = 128, K = 5; and a
    single-stream handle takes [frames, M]"""
    M, K, S = 128, 5, 2
    blocks = blocks_a(K)
    g, X, ref = white_case(M, taps_len(M, K), S, sum(blocks))
    sy = tuned(g, M, S, C64, kernel, 3)
    cuts = np.cumsum([0] + blocks)
    y = np.concatenate([sy.execute_block(X[:, a:b]) for a, b in zip(cuts[:-1], cuts[1:])], axis=1)
    check_streams(y, ref, M, 1e-6, f"G host blocks M={M} K={K} S={S} kernel={kernel}")
    one = tuned(g, M, 1, C64, kernel, 3)
    y0 = np.concatenate([one.execute_block(X[0, a:b]) for a, b in zip(cuts[:-1], cuts[1:])])
    assert y0.shape == (sum(blocks) * M,) and bits_equal(y0, y[0])


@gpu
@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("M,K", [(32, 5), (1024, 2)])
def test_8_byte_aligned_blocks(M, K, kernel):
    """input and output each one complex64 past a 16-byte boundary: the same bits as aligned blocks"""
    blocks = blocks_a(K)
    g, X, ref = white_case(M, taps_len(M, K), S3, sum(blocks))
    y = run_blocks(tuned(g, M, S3, C64, kernel, 3), X, blocks, in_off=1, out_off=1)
    check_streams(y, ref, M, 1e-6, f"G 8-byte aligned M={M} K={K} kernel={kernel}")
    assert bits_equal(y, run_case(M, K, C64, kernel, 3))


@gpu
@pytest.mark.parametrize("kernel", [1, 2])
def test_refused_calls_leave_the_state_untouched(kernel):
    """n % M != 0 and overlapping input and output are refused with SDSP_E_INVALID_ARGUMENT; the next valid
    call equals an undisturbed handle's, bit for bit.  n = 0 returns 0 frames and changes nothing"""
    import torch
    M, K, S = 64, 4, 2
    g = white_taps(M * K)
    X = white_frames(S, 9, M)
    st = torch.cuda.current_stream()

    def call(sy, a, b):
        d_in = to_dev(np.ascontiguousarray(X[:, a:b]).reshape(-1))
        d_out = empty_dev(S * (b - a) * M, C64)
        assert sy.execute_block_device(d_in, (b - a) * M, d_out, st) == b - a
        return to_host(d_out)

    calm, poked = tuned(g, M, S, C64, kernel, 2), tuned(g, M, S, C64, kernel, 2)
    assert bits_equal(call(calm, 0, 4), call(poked, 0, 4))
    d_in, d_out = to_dev(np.ascontiguousarray(X[:, 4:9]).reshape(-1)), empty_dev(S * 5 * M, C64)
    for n in (M + 1, M - 1, 5 * M - 3):
        with pytest.raises(sd.SdspError) as e:
            poked.execute_block_device(d_in, n, d_out, st)
        assert e.value.code == E_INVALID_ARGUMENT and "whole number" in str(e.value)
    for out in (d_in, d_in[M:]):  # the same block; a block that starts inside the input
        with pytest.raises(sd.SdspError) as e:
            poked.execute_block_device(d_in, 2 * M, out, st)
        assert e.value.code == E_INVALID_ARGUMENT and "overlap" in str(e.value)
    # the host entry point refuses a ragged n before it reads the block
    assert sd.lib().sdsp_ichan_execute_block(poked._h, None, M + 1, None, None) == E_INVALID_ARGUMENT
    assert poked.execute_block_device(d_in, 0, d_out, st) == 0
    assert bits_equal(call(calm, 4, 9), call(poked, 4, 9))


@gpu
@pytest.mark.parametrize("kernel", [1, 2])
def test_reset_and_set_streams_zero_the_history(kernel):
    M, K, S = 64, 4, 2
    g = white_taps(M * K)
    X = white_frames(S, 6, M)
    fresh = tuned(g, M, S, C64, kernel, 2).execute_block(X[:, 3:])
    assert not bits_equal(fresh, tuned(g, M, S, C64, kernel, 2).execute_block(X)[:, 3 * M:])  # the history matters
    sy = tuned(g, M, S, C64, kernel, 2)
    sy.execute_block(X[:, :3])
    sy.reset()
    assert bits_equal(sy.execute_block(X[:, 3:]), fresh)
    sy.set_streams(1)
    sy.execute_block(X[0, :3])
    sy.set_streams(S)
    assert bits_equal(sy.execute_block(X[:, 3:]), fresh)
