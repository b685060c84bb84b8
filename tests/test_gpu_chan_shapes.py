"""The PFB + FFT channeliser at every branch depth, channel count and block shape, against a plain
complex128 restatement, on inputs that weigh every (branch, tap) pair.

The channeliser tests of test_gpu_fft.py use firdes_kaiser(M K, 0.5 / M, 80, 0) taps.  That design is
symmetric: reversing the whole tap vector (branch p <-> M-1-p together with tap i <-> K-1-i) leaves
the output unchanged, and their second bound, 1e-6 sum|h| max|x| sqrt(M), is 500 (M = 64) to 8000
(M = 1024) times what f32 arithmetic needs (test_what_the_inputs_see prints both).  Here:

- white taps: default_rng(TAP_SEED).standard_normal(len) in the handle's precision;
- white streams from O.synth;
- impulse streams: zeros and single samples of 0.75 - 0.5j, whose response is known in closed form
  and outside of which every output is exactly zero.

Reference: chan_ref below (numpy complex128; np.fft.fft, not the oracle's FFT, whose DFT16 constants
limit agreement to 1e-7), pinned on the CPU to orc_channelize and to the committed fixture.
Tolerance, per stream, tol = 1e-6 for complex64 (section 8d) and 1e-12 for complex128 (the figure of
test_fft_large_and_any_size against numpy):
    rel_rms(y, ref) <= tol   and   for every frame m  ||y[m] - ref[m]|| <= tol sqrt(mean_m ||ref[m]||^2)
test_f32_arithmetic_alone_stays_inside shows on the CPU that f32 arithmetic in the reference's own
order stays below half of both.
"""
import functools
import os
import sys

import numpy as np
import pytest

import oracle_lib as O
from gpu_util import bits_equal, empty_dev, rel_rms, to_dev, to_host

gpu = pytest.mark.gpu

sd = pytest.importorskip("solid_dsp_amd")
from solid_dsp_amd import Channelizer  # noqa: E402

F32, F64, C64, C128 = np.float32, np.float64, np.complex64, np.complex128
SEED = 20261020      # streams
TAP_SEED = 20261021  # white taps
AMP = 0.75 - 0.5j    # the impulse: exact in f32
TUNE_STREAMING, TUNE_FPB, TUNE_XCD = 8, 9, 15  # SDSP_TUNE_CHAN_STREAMING, _FRAMES_PER_BLOCK, _XCD_ORDER
TOL = {C64: 1e-6, C128: 1e-12}


def coef_dtype(prec):
    return F32 if prec == C64 else F64


# ---------------------------------------------------------------- reference and inputs
def chan_ref(h, M, x, prec=C64):
    """v_p[m] = sum_{i<K} h[p + (K-1-i) M] x[(m-i) M + (M-1-p)],  X[m] = fft(v[m]),  x[<0] = 0,
    K = len(h) // M (later taps ignored); taps and samples rounded to `prec`, then complex128.
    [frames, M]"""
    K = len(h) // M
    frames = len(x) // M
    hb = np.asarray(h)[:K * M].astype(coef_dtype(prec)).astype(F64).reshape(K, M)  # hb[idx][p] = h[p + idx M]
    xx = np.concatenate([np.zeros((K - 1) * M, C128), np.asarray(x)[:frames * M].astype(prec).astype(C128)])
    xr = xx.reshape(frames + K - 1, M)[:, ::-1]  # xr[f + K-1][p] = x[f M + M-1-p]
    v = np.zeros((frames, M), C128)
    for i in range(K):
        v += hb[K - 1 - i][None, :] * xr[K - 1 - i:K - 1 - i + frames]
    return np.fft.fft(v, axis=1)


def chan_f32(h, M, x):
    """the same sums in numpy float32 and scipy's single-precision FFT: what f32 arithmetic in the
    reference's order gives"""
    import scipy.fft
    K = len(h) // M
    frames = len(x) // M
    hb = np.asarray(h)[:K * M].astype(F32).reshape(K, M)
    xx = np.concatenate([np.zeros((K - 1) * M, C64), np.asarray(x)[:frames * M].astype(C64)])
    xr = xx.reshape(frames + K - 1, M)[:, ::-1]
    v = np.zeros((frames, M), C64)
    for i in range(K):
        v += hb[K - 1 - i][None, :] * xr[K - 1 - i:K - 1 - i + frames]
    assert v.dtype == C64
    y = scipy.fft.fft(v, axis=1)
    assert y.dtype == C64
    return y


@functools.lru_cache(maxsize=None)
def white_taps(n, prec=C64, seed=TAP_SEED):
    h = np.random.default_rng(seed).standard_normal(n).astype(coef_dtype(prec))
    h.setflags(write=False)
    return h


@functools.lru_cache(maxsize=None)
def streams(S, n, prec=C64, first=0):
    x = np.stack([O.synth(SEED, first + s, 0, n, complex_=True) for s in range(S)]).astype(prec)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def white_case(M, ntaps, S, frames, prec=C64):
    """(taps, [S, frames M] streams, [S, frames, M] reference), shared by the cases of one shape"""
    h = white_taps(ntaps, prec)
    x = streams(S, M * frames, prec)
    ref = np.stack([chan_ref(h, M, x[s], prec) for s in range(S)])
    ref.setflags(write=False)
    return h, x, ref


# ---------------------------------------------------------------- the two criteria
def figures(y, ref):
    """(whole-output rel-RMS, worst frame error over the RMS frame norm) of one stream [frames, M]"""
    y, ref = np.asarray(y).astype(C128), np.asarray(ref)
    err = np.linalg.norm(y - ref, axis=-1)
    rms_frame = float(np.sqrt(np.mean(np.linalg.norm(ref, axis=-1) ** 2)))
    return rel_rms(y, ref), float(err.max()) / rms_frame, int(err.argmax())


def check_streams(y, ref, tol, what):
    """both criteria on every stream of [S, frames, M]; prints the worst figures of the case"""
    assert y.shape == ref.shape, (y.shape, ref.shape)
    figs = [figures(y[s], ref[s]) for s in range(len(ref))]
    whole, frame = max(f[0] for f in figs), max(f[1] for f in figs)
    print(f"{what}: whole {whole:.3e}, frame {frame:.3e} (limit {tol:.0e})")
    for s, (w, f, m) in enumerate(figs):
        assert w <= tol, f"{what}: stream {s} rel-RMS {w:.3e} > {tol:.0e}"
        assert f <= tol, f"{what}: stream {s} frame {m} is off by {f:.3e} of the RMS frame norm > {tol:.0e}"
    return whole, frame


# ---------------------------------------------------------------- CPU: the reference and the inputs
@pytest.mark.parametrize("M,K", [(16, 4), (1024, 3), (64, 8)])
def test_chan_ref_matches_restatement(M, K):
    """chan_ref against orc_channelize (f64 taps, complex128 samples), white taps with a tail that
    must be ignored, 12 frames: rel-RMS <= 1e-7, the oracle FFT's own accuracy"""
    frames = 12
    h = white_taps(M * K + M // 2 + 1, C128)
    x = streams(1, M * frames, C128)[0]
    ref = np.zeros(M * frames, C128)
    O.lib().orc_channelize(O._ptr(np.ascontiguousarray(h[:M * K])), M * K, M, O._ptr(np.ascontiguousarray(x)),
                           len(x), O._ptr(ref))
    rel = rel_rms(chan_ref(h, M, x, C128), ref.reshape(frames, M))
    print(f"chan_ref vs orc_channelize M={M} K={K}: rel-RMS {rel:.3e}")
    assert rel <= 1e-7


def test_chan_ref_matches_fixture():
    """chan_ref against the committed chan_m64_k8 vectors (complex128 y: 1e-7)"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden as G
    kind, p, a = G.load("chan_m64_k8")
    assert kind == "chan" and a["y"].dtype == C128
    rel = rel_rms(chan_ref(a["taps"], p["M"], a["x"], C128).reshape(-1), a["y"])
    print(f"chan_ref vs fixture chan_m64_k8: rel-RMS {rel:.3e}")
    assert rel <= 1e-7


@pytest.mark.parametrize("M,K", [(64, 8), (1024, 8)])
def test_what_the_inputs_see(M, K):
    """the reversed tap vector under chan_ref: the Kaiser design of the older tests gives the same
    output (<= 1e-12), white taps a different one (> 1); and the share of the older max-abs bound
    1e-6 sum|h| max|x| sqrt(M) that f32 arithmetic uses"""
    frames = 45
    x = streams(1, M * frames)[0]
    kaiser = O.firdes_kaiser(M * K, 0.5 / M, 80.0, 0.0).astype(F32)
    moved = {}
    for kind, h in (("kaiser", kaiser), ("white", white_taps(M * K))):
        ref = chan_ref(h, M, x)
        moved[kind] = rel_rms(chan_ref(h[::-1].copy(), M, x), ref)
        err = float(np.abs(chan_f32(h, M, x).astype(C128) - ref).max())
        bound = 1e-6 * float(np.abs(h.astype(F64)).sum()) * float(np.abs(x).max()) * np.sqrt(M)
        print(f"M={M} K={K} {kind} taps: reversal moves the output by {moved[kind]:.3e} rel-RMS; "
              f"f32 arithmetic uses {err / bound:.1e} of the max-abs bound")
    assert moved["kaiser"] <= 1e-12
    assert moved["white"] > 1


@pytest.mark.parametrize("K", [1, 8, 12])
@pytest.mark.parametrize("M", [4, 64, 1024, 4096])
def test_f32_arithmetic_alone_stays_inside(M, K):
    """f32 branch sums and a single-precision FFT on the CPU, white taps and stream, 45 frames: both
    criteria at half their limit (measured over M = 4 .. 4096, K = 1 .. 12: per frame at most 1.9e-7,
    whole output at most 1.4e-7)"""
    frames = 45
    h = white_taps(M * K)
    x = streams(1, M * frames)[0]
    check_streams(chan_f32(h, M, x)[None], chan_ref(h, M, x)[None], 5e-7, f"f32 on the CPU M={M} K={K}")


# ---------------------------------------------------------------- GPU helpers
def offset_view(count, prec, off):
    """a device buffer of `count` samples whose address is `off` samples past an allocation"""
    return empty_dev(count + off, prec)[off:]


def run_blocks(ch, x, blocks, in_off=0, out_off=0):
    """feed [S, frames M] through execute_block_device in calls of blocks[i] frames on the current
    stream; [S, frames, M]"""
    import torch
    S, M, prec = x.shape[0], ch.M, x.dtype.type
    assert sum(blocks) * M == x.shape[1]
    st = torch.cuda.current_stream()
    y = np.zeros((S, sum(blocks), M), prec)
    a = 0
    for nb in blocks:
        b = a + nb
        d_in = offset_view(S * nb * M, prec, in_off)
        d_in.copy_(to_dev(np.ascontiguousarray(x[:, a * M:b * M]).reshape(-1)))
        d_out = offset_view(S * nb * M, prec, out_off)
        if prec == C64:
            assert d_in.data_ptr() % 16 == 8 * in_off and d_out.data_ptr() % 16 == 8 * out_off
        assert ch.execute_block_device(d_in, nb * M, d_out, st) == nb
        y[:, a:b] = to_host(d_out).reshape(S, nb, M)
        a = b
    return y


def tuned(h, M, S, prec=C64, variant=None, fpb=None, xcd=None):
    ch = Channelizer(h, M, sample_dtype=prec, streams=S)
    for key, v in ((TUNE_STREAMING, variant), (TUNE_FPB, fpb), (TUNE_XCD, xcd)):
        if v is not None:
            ch.set_tuning(key, v)
    return ch


def name(prec):
    return "c64" if prec == C64 else "c128"


# ================================================================ A. the generic kernel
def blocks_a(K):
    return [1, K + 2, 2, 4]  # a one-frame block; blocks shorter than the K-1 history frames; four calls


def taps_len(M, K):
    return M * K + (M // 2 + 1 if K == 5 else 0)  # K = 5: a tail that must be ignored


GENERIC = [(M, C64) for M in (4, 8, 32, 128, 256, 512, 2048, 4096)] + \
          [(M, C128) for M in (4, 8, 32, 128, 256, 512, 1024, 2048, 4096)]


def test_generic_cases_reach_every_workgroup_size():
    """launch_chan_t, restated: 64 threads below M = 256, M / 4 at 256 and 512, 256 from 1024 up; the
    cases of test_generic_every_channel_count reach each in both precisions (complex64 at M = 1024
    runs chan_kernel<float> in test_generic_1024_more_than_8_taps)"""
    def threads(M):
        return 256 if M >= 1024 else (M // 4 if M >= 256 else 64)
    for prec in (C64, C128):
        got = {threads(M) for M, p in GENERIC if p == prec} | ({256} if prec == C64 else set())
        assert got == {64, 128, 256}


@gpu
@pytest.mark.parametrize("K", [1, 2, 5])
@pytest.mark.parametrize("M,prec", GENERIC, ids=[f"{M}-{name(p)}" for M, p in GENERIC])
def test_generic_every_channel_count(M, prec, K):
    """chan_kernel<float> / <double> at every M (all three workgroup sizes of launch_chan_t), K = 1
    (no history), 2 and 5 (with a tap tail), three streams, blocks of 1, K + 2, 2 and 4 frames"""
    blocks = blocks_a(K)
    h, x, ref = white_case(M, taps_len(M, K), 3, sum(blocks), prec)
    y = run_blocks(tuned(h, M, 3, prec), x, blocks)
    check_streams(y, ref, TOL[prec], f"A generic M={M} K={K} {name(prec)}")


@gpu
def test_generic_host_blocks_two_streams():
    """execute_block with a host [2, n] array per call (the staged multi-stream path), M = 128, K = 5"""
    M, K, S = 128, 5, 2
    blocks = blocks_a(K)
    h, x, ref = white_case(M, taps_len(M, K), S, sum(blocks))
    ch = Channelizer(h, M, sample_dtype=C64, streams=S)
    cuts = np.cumsum([0] + blocks) * M
    y = np.concatenate([ch.execute_block(x[:, a:b]) for a, b in zip(cuts[:-1], cuts[1:])], axis=1)
    check_streams(y, ref, 1e-6, f"A generic host blocks M={M} K={K} S={S}")


# ================================================================ B. M = 1024, K > 8
@gpu
@pytest.mark.parametrize("K", [9, 12])
def test_generic_1024_more_than_8_taps(K):
    """M = 1024 complex64 with the streaming knob at its default and K > 8: no chan1024_kernel<K>
    exists, chan_kernel<float> must run and be right"""
    M, blocks = 1024, blocks_a(K)
    h, x, ref = white_case(M, M * K, 3, sum(blocks))
    y = run_blocks(tuned(h, M, 3), x, blocks)
    check_streams(y, ref, 1e-6, f"B M=1024 K={K} default knobs")


# ================================================================ C. every streaming instantiation
BLOCKS_C = [3, 21, 1, 20]


def chunk_map(frames, S, variant, fpb, xcd):
    """try_launch_chan1024_t, restated: (frames per chunk, chunks per stream, chunks, workgroups,
    XCD order in effect)"""
    R = 8 if variant in (2, 4, 5, 6) else 16
    Fd = min(max(frames * S // 512, 64), 256)
    F = ((fpb if fpb > 0 else Fd) + R - 1) // R * R
    cps = (frames + F - 1) // F
    C = cps * S
    G = min(C, 512 if variant in (2, 4) else 256)
    if xcd:
        G = G // 8 * 8
        if G == 0:
            xcd, G = 0, C
    return F, cps, C, G, xcd


def test_streaming_cases_reach_what_they_name():
    """the chunk geometry of groups C and D, from the launcher's arithmetic"""
    for v in range(1, 7):
        F = 8 if v in (2, 4, 5, 6) else 16
        assert chunk_map(21, 3, v, 8, 1)[0] == F
    # 8-frame chunks, XCD order: 9 chunks on 8 workgroups with windows of 2; workgroup 4 is clipped to
    # one chunk, 5 .. 7 have none
    assert chunk_map(21, 3, 5, 8, 1) == (8, 3, 9, 8, 1)
    assert chunk_map(21, 3, 5, 8, 0) == (8, 3, 9, 9, 0)
    assert chunk_map(21, 3, 3, 8, 1) == (16, 2, 6, 6, 0)  # fewer than 8 chunks: launch order
    assert chunk_map(21, 3, 5, 5, 1)[0] == 8 and chunk_map(21, 3, 3, 5, 1)[0] == 16  # 5 rounds up
    assert chunk_map(21, 3, 4, 4096, 1) == (4096, 1, 3, 3, 0)
    # default knobs, 11 streams: 11 chunks (not a multiple of 8), then 22 chunks of 64 frames
    assert chunk_map(10, 11, 5, 0, 1) == (64, 1, 11, 8, 1)
    assert chunk_map(70, 11, 5, 0, 1) == (64, 2, 22, 16, 1)


@gpu
@pytest.mark.parametrize("xcd", [0, 1])
@pytest.mark.parametrize("variant", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 6, 7, 8])
def test_streaming_every_instantiation(K, variant, xcd):
    """chan1024_kernel<K, ...> for K = 1 .. 8 on each of the six forms, chunks of 8 frames (16 on
    forms 1 and 3), three streams, blocks of 3, 21, 1 and 20 frames: a first call shorter than K - 1
    frames (K >= 5: the warm-up of the next call mixes history and input), chunk boundaries inside a
    call, ragged last rounds, a one-frame call; with XCD order the 21-frame call has 9 chunks on 8
    workgroups"""
    M, S = 1024, 3
    h, x, ref = white_case(M, M * K, S, sum(BLOCKS_C))
    y = run_blocks(tuned(h, M, S, variant=variant, fpb=8, xcd=xcd), x, BLOCKS_C)
    check_streams(y, ref, 1e-6, f"C streaming K={K} variant={variant} xcd={xcd}")


@gpu
@pytest.mark.parametrize("fpb", [5, 4096])
@pytest.mark.parametrize("variant", [3, 4, 5])
@pytest.mark.parametrize("K", [2, 7])
def test_streaming_odd_and_huge_chunks(K, variant, fpb):
    """frames per chunk 5 (rounded up to a whole round) and 4096 (one chunk per stream: fewer than 8
    chunks, so the XCD map falls back to launch order), XCD order requested"""
    M, S = 1024, 3
    h, x, ref = white_case(M, M * K, S, sum(BLOCKS_C))
    y = run_blocks(tuned(h, M, S, variant=variant, fpb=fpb, xcd=1), x, BLOCKS_C)
    check_streams(y, ref, 1e-6, f"C streaming K={K} variant={variant} fpb={fpb}")


# ================================================================ D. default knobs on the XCD path
@gpu
@pytest.mark.parametrize("K", [4, 8])
def test_default_knobs_xcd_path(K):
    """no set_tuning: 11 streams, blocks of 10 and 70 frames: 11 chunks on 8 workgroups (the last
    XCD windows clipped and empty), then 22 chunks of 64 frames with a ragged last round"""
    M, S, blocks = 1024, 11, [10, 70]
    h, x, ref = white_case(M, M * K, S, sum(blocks))
    y = run_blocks(Channelizer(h, M, sample_dtype=C64, streams=S), x, blocks)
    check_streams(y, ref, 1e-6, f"D default knobs K={K} S={S}")


# ================================================================ E. 8-byte aligned blocks
@gpu
@pytest.mark.parametrize("out_off", [0, 1])
@pytest.mark.parametrize("variant", [2, 4, 5, 0])
@pytest.mark.parametrize("K", [3, 8])
def test_input_only_8_byte_aligned(K, variant, out_off):
    """the input one complex64 past a 16-byte boundary (and the output too, out_off = 1): the
    512-thread forms 2 and 4 load 16 bytes per lane and must fall back to form 1, bit-identical to a
    fresh handle on form 1 fed the same views; the default form 5 and the per-frame kernel (0) take
    such input as it is"""
    M, S = 1024, 3
    h, x, ref = white_case(M, M * K, S, sum(BLOCKS_C))
    y = run_blocks(tuned(h, M, S, variant=variant, fpb=8), x, BLOCKS_C, in_off=1, out_off=out_off)
    check_streams(y, ref, 1e-6, f"E 8-byte aligned K={K} variant={variant} out_off={out_off}")
    if variant in (2, 4):
        y1 = run_blocks(tuned(h, M, S, variant=1, fpb=8), x, BLOCKS_C, in_off=1, out_off=out_off)
        assert bits_equal(y, y1), f"form {variant} on 8-byte aligned input differs from form 1"


# ================================================================ F. impulses
BLOCKS_F = [20, 30]


def impulse_sites(M, K):
    """(frame, position in the frame) of the impulses, at least K + 1 frames apart, for blocks of 20
    and 30 frames and chunks of 8 or 16 frames: the stream's first sample; the last sample of a frame;
    the frame before the block boundary (the response arrives through the history); the frame before
    the chunk boundary at frame 16 of the second block (through the warm-up loads); and max(K - 2, 1)
    frames before the end (the response is cut short)"""
    total = sum(BLOCKS_F)
    sites = [(0, 0), (10, M - 1), (BLOCKS_F[0] - 1, 5 % M), (BLOCKS_F[0] + 15, 300 % M), (total - max(K - 2, 1), M // 2)]
    fr = [f for f, _ in sites]
    assert all(b - a >= K + 1 for a, b in zip(fr[:-1], fr[1:])), fr
    assert fr[-1] + K > total  # cut short
    return sites


def impulse_case(M, K, prec, S, s0, what, **knobs):
    """impulses of AMP on stream s0, zeros elsewhere: frame m0 + i, i < K, of stream s0 is
    AMP h[p + (K-1-i) M] exp(-2j pi p k / M) with p = M-1 - q % M, m0 = q // M, each within tol of its
    own norm; every other output of every stream is exactly zero"""
    total, tol = sum(BLOCKS_F), TOL[prec]
    h = white_taps(M * K, prec)
    x = np.zeros((S, M * total), prec)
    expect = {}
    for m0, r in impulse_sites(M, K):
        x[s0, m0 * M + r] = AMP
        p = M - 1 - r
        for i in range(K):
            if m0 + i < total:
                assert m0 + i not in expect
                expect[m0 + i] = AMP * float(h[p + (K - 1 - i) * M]) * np.exp(-2j * np.pi * ((p * np.arange(M)) % M) / M)
    y = run_blocks(tuned(h, M, S, prec, **knobs), x, BLOCKS_F)
    silent = np.ones((S, total), bool)
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


@gpu
@pytest.mark.parametrize("variant", [0, 1, 2, 3, 4, 5, 6])
def test_impulses_1024_every_form(variant):
    """M = 1024, K = 8, three streams with the impulses on the middle one, chunks of 8 (16) frames"""
    impulse_case(1024, 8, C64, 3, 1, f"F impulses M=1024 K=8 variant={variant}", variant=variant, fpb=8)


@gpu
def test_impulses_1024_five_taps():
    impulse_case(1024, 5, C64, 3, 1, "F impulses M=1024 K=5 variant=4", variant=4, fpb=8)


@gpu
@pytest.mark.parametrize("M,K,prec", [(16, 3, C64), (512, 4, C128), (4096, 2, C64)],
                         ids=["16-3-c64", "512-4-c128", "4096-2-c64"])
def test_impulses_generic(M, K, prec):
    impulse_case(M, K, prec, 3, 1, f"F impulses generic M={M} K={K} {name(prec)}")
