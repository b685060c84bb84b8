"""The spectrometer (solid_dsp_amd.Spectrometer, sdsp_spec_*) on the device: bit for bit against
sd.OversampledChannelizer behind the numpy fold (tests/spec_cases.py spec_fold) on both kernels at every
workgroup shape, branch depth, frame-stride class and integration class; across call splits; through the
fold kernel's longest sum; against the complex128 definition; against closed forms; and at its boundary.

Inputs (tests/test_spec_capi.py shows on the CPU what they can see): white taps, white streams from
O.synth, three streams, 230 frames per stream fed through execute_block_device in calls of 1, 2, 8, 34, 31,
32, 33 and 89 frames, every output filled with NaN first between guard elements; filled, phase and the
returned count are checked after every call.  Tolerance (section 8d), per stream and per spectrum:
||P_j - Pref_j|| <= tol ||Pref_j||, tol = 1e-6 for complex64 and 1e-12 for complex128;
test_f32_arithmetic_alone_stays_inside (test_spec_capi.py) shows f32 arithmetic alone below half of it.
"""
import functools

import numpy as np
import pytest

from gpu_util import bits_equal, empty_dev, to_dev, to_host
from spec_cases import (BLOCKS, C64, C128, DEFINITION, F32, F64, FRAMES, MAX_A, S3, SETTINGS, SHAPES, SHAPE_IDS, TOL,
                        TUNE_KERNEL, TUNE_SUBBLOCKS, coef_dtype, name, slide_fits, spec_fold, spec_plan, spec_ref,
                        taps_len, white_input, white_streams, white_taps)

gpu = pytest.mark.gpu

sd = pytest.importorskip("solid_dsp_amd")

E_INVALID_ARGUMENT = 90
GUARD = 4        # elements either side of every output (16 bytes in f32: the alignment stays)
SENTINEL = -7.0


# ---------------------------------------------------------------- helpers
def tuned(h, M, D, A, S, prec=C64, kernel=None, sub=None):
    sp = sd.Spectrometer(h, M, D, A, sample_dtype=prec, streams=S)
    for key, v in ((TUNE_KERNEL, kernel), (TUNE_SUBBLOCKS, sub)):
        if v is not None:
            sp.set_tuning(key, v)
    return sp


def call(sp, xb, frames_before, in_off=0, out_off=0, stream=None):
    """one execute_block_device call on [S, nb D] samples: the input `in_off` samples and the output
    `out_off` reals past an allocation, the output NaN between guards, a null output when the call
    emits nothing; filled, phase and the count are checked.  [S, spectra, M]"""
    import torch
    S, n = xb.shape
    M, D, A = sp.M, sp.D, sp.A
    prec, T = xb.dtype.type, coef_dtype(xb.dtype.type)
    nb, filled = n // D, frames_before % A
    want, left = divmod(filled + nb, A)
    assert sp.filled == filled and sd.Spectrometer.count(D, A, filled, n) == (want, left)
    d_in = empty_dev(S * n + in_off, prec)[in_off:]
    d_in.copy_(to_dev(np.ascontiguousarray(xb).reshape(-1)))
    count = S * want * M
    d_all = empty_dev(out_off + 2 * GUARD + count, T)
    d_all.fill_(SENTINEL)
    d_out = d_all[out_off + GUARD:out_off + GUARD + count]
    d_out.fill_(float("nan"))
    if prec == C64:
        assert d_in.data_ptr() % 16 == (8 * in_off) % 16
        assert not count or d_out.data_ptr() % 16 == (4 * out_off) % 16
    st = stream if stream is not None else torch.cuda.current_stream()
    assert sp.execute_block_device(d_in, n, d_out if want else None, st) == want
    total = frames_before + nb
    assert sp.filled == left and sp.phase == (total * D) % M, (sp.filled, sp.phase, total)
    everything = to_host(d_all)
    edges = np.concatenate([everything[:out_off + GUARD], everything[out_off + GUARD + count:]])
    assert np.all(edges == SENTINEL), "a guard element was written"
    return everything[out_off + GUARD:out_off + GUARD + count].reshape(S, want, M)


def run_blocks(sp, x, blocks, **kw):
    """[S, frames D] through `call` in calls of blocks[i] frames; [S, J, M]"""
    D, a, out = sp.D, 0, []
    assert sum(blocks) * D == x.shape[1]
    for nb in blocks:
        out.append(call(sp, x[:, a * D:(a + nb) * D], a, **kw))
        a += nb
    y = np.concatenate(out, axis=1)
    assert not np.isnan(y).any()
    return y


@functools.lru_cache(maxsize=8)
def oschan_frames(M, K, D, prec, frames=FRAMES, blocks=tuple(BLOCKS), S=S3):
    """the oversampled channeliser's frames on the same calls; [S, frames, M]"""
    import torch
    h, x = white_input(M, K, D, prec, frames, S)
    ch = sd.OversampledChannelizer(h, M, D, sample_dtype=prec, streams=S)
    st, a, out = torch.cuda.current_stream(), 0, []
    for nb in blocks:
        d_out = empty_dev(S * nb * M, prec)
        ch.execute_block_device(to_dev(np.ascontiguousarray(x[:, a * D:(a + nb) * D]).reshape(-1)), nb * D, d_out, st)
        out.append(to_host(d_out).reshape(S, nb, M))
        a += nb
    return np.concatenate(out, axis=1)


def folded(Y, A, blocks, T, scale=1.0):
    """spec_fold call by call on the channeliser's frames, the state carried in numpy; [S, J, M]"""
    state, a, out = (0, None, None), 0, []
    for nb in blocks:
        sp, *state = spec_fold(Y[:, a:a + nb], A, *state, scale, T)
        out.append(sp)
        a += nb
    return np.concatenate(out, axis=1)


def settings_of(M, K, D, prec):
    return [(k, r) for k, r in SETTINGS if k == 1 or slide_fits(M, K, D, prec)]


def check_info(sp, M, K, D, A, prec, kernel, sub):
    want = spec_plan(M, K, D, A, prec, kernel, sub)
    assert sp.info() == want, f"info() {sp.info()}, the restated plan gives {want}"
    assert (sp.M, sp.D, sp.A, sp.K, sp.phase, sp.filled) == (M, D, A, K, 0, 0)


def spectrum_errors(P, ref):
    """worst ||P_j - ref_j|| / ||ref_j|| over streams and spectra"""
    P, ref = np.asarray(P, F64), np.asarray(ref, F64)
    assert P.shape == ref.shape, (P.shape, ref.shape)
    return float((np.linalg.norm(P - ref, axis=-1) / np.linalg.norm(ref, axis=-1)).max())


# ================================================================ a. bit for bit against the handle it fuses
@gpu
@pytest.mark.parametrize("M,K,D,A,prec", SHAPES, ids=SHAPE_IDS)
def test_bit_identical_to_the_channeliser_behind_the_fold(M, K, D, A, prec):
    """sd.OversampledChannelizer on the same calls, its frames through spec_fold with the state carried
    in numpy: the per-frame kernel at 1 and 3 sub-blocks per workgroup and, where it fits, the sliding
    kernel at automatic, 1 and 3 give those bits, so all settings of a shape are bit-identical"""
    h, x = white_input(M, K, D, prec)
    want = folded(oschan_frames(M, K, D, prec), A, BLOCKS, coef_dtype(prec))
    assert want.shape == (S3, FRAMES // A, M)
    for kernel, sub in settings_of(M, K, D, prec):
        sp = tuned(h, M, D, A, S3, prec, kernel, sub)
        check_info(sp, M, K, D, A, prec, kernel, sub)
        got = run_blocks(sp, x, BLOCKS)
        assert bits_equal(got, want), \
            f"M={M} K={K} D={D} A={A} {name(prec)} kernel {kernel} at {sub} sub-blocks: " \
            f"{int(np.count_nonzero(got != want))} of {want.size} values differ from the channeliser behind the fold"


@gpu
def test_the_calls_reach_every_kind():
    """of the eight calls, at A = 100: the first closes no sub-block, the fourth closes one and no
    integration, and the first five emit nothing (a null output); at A = 5 the last closes 18 integrations"""
    ends = [int(e) for e in np.cumsum(BLOCKS)]
    assert ends[0] < 32 and ends[2] < 32 <= ends[3] < 100 and ends[5] >= 100 > ends[4]
    assert sd.Spectrometer.count(1, 100, 0, ends[4]) == (0, 76)
    assert sd.Spectrometer.count(1, 5, ends[6] % 5, 89) == (18, 0)
    h, x = white_input(64, 8, 48)
    sp = tuned(h, 64, 48, 100, S3)
    assert sp.execute_block_device(to_dev(np.ascontiguousarray(x[:, :48]).reshape(-1)), 48, None) == 0
    with pytest.raises(sd.SdspError) as e:  # a call that emits a spectrum needs an output
        sp.execute_block_device(to_dev(np.ascontiguousarray(x[:, :99 * 48]).reshape(-1)), 99 * 48, None)
    assert e.value.code == E_INVALID_ARGUMENT and sp.filled == 1


# ================================================================ b. call splits
@gpu
@pytest.mark.parametrize("kernel,sub", [(1, 0), (2, 0), (2, 3)])
@pytest.mark.parametrize("A", [5, 33])
def test_one_frame_per_call(A, kernel, sub):
    """M = 64, 130 frames fed in one call, in ragged calls and one frame per call: the same bits"""
    M, K, D, frames = 64, 8, 48, 130
    h, x = white_input(M, K, D, C64, frames)
    whole = run_blocks(tuned(h, M, D, A, S3, C64, kernel, sub), x, [frames])
    assert whole.shape == (S3, frames // A, M)
    for blocks in ([1, 2, 8, 34, 31, 32, 22], [1] * frames):
        assert bits_equal(run_blocks(tuned(h, M, D, A, S3, C64, kernel, sub), x, blocks), whole), len(blocks)


@gpu
@pytest.mark.parametrize("M,K,D,A,prec", [(1024, 3, 1000, 32, C64), (256, 1, 128, 33, C128), (4096, 1, 4096, 100, C64),
                                          (4, 12, 3, 65, C64)])
def test_one_call_is_the_ragged_calls(M, K, D, A, prec):
    h, x = white_input(M, K, D, prec)
    want = folded(oschan_frames(M, K, D, prec), A, BLOCKS, coef_dtype(prec))
    for kernel, sub in settings_of(M, K, D, prec):
        assert bits_equal(run_blocks(tuned(h, M, D, A, S3, prec, kernel, sub), x, [FRAMES]), want), (kernel, sub)


# ================================================================ c. the longest fold
LONG_BLOCKS = (30000, 1, 35535, 1000)  # two integrations of 32768 frames and an open tail


@gpu
@pytest.mark.parametrize("M,K,D,prec", [(4, 3, 1, C64), (4, 1, 3, C128), (8, 1, 1, C128), (8, 3, 3, C64)],
                         ids=["4-3-1-c64", "4-1-3-c128", "8-1-1-c128", "8-3-3-c64"])
def test_longest_fold(M, K, D, prec):
    """A = 32768: the fold kernel's 1024 steps, twice, the second integration starting inside a call
    and 1000 frames left open; the bit comparison of (a)"""
    frames, S = sum(LONG_BLOCKS), 2
    assert frames == 2 * MAX_A + 1000
    h, x = white_input(M, K, D, prec, frames, S)
    want = folded(oschan_frames(M, K, D, prec, frames, LONG_BLOCKS, S), MAX_A, LONG_BLOCKS, coef_dtype(prec))
    assert want.shape == (S, 2, M)
    for kernel, sub in ((1, 0), (2, 0), (2, 3)):
        sp = tuned(h, M, D, MAX_A, S, prec, kernel, sub)
        got = run_blocks(sp, x, list(LONG_BLOCKS))
        assert sp.filled == 1000
        assert bits_equal(got, want), (kernel, sub, got, want)


# ================================================================ d. the definition
@gpu
@pytest.mark.parametrize("M,K,D,A,prec", DEFINITION, ids=[f"{M}-{K}-{D}-A{A}-{name(p)}" for M, K, D, A, p in DEFINITION])
def test_against_the_definition(M, K, D, A, prec):
    h, x = white_input(M, K, D, prec)
    ref = np.stack([spec_ref(h, M, D, A, x[s], prec) for s in range(S3)])
    for kernel in (1, 2):
        got = run_blocks(tuned(h, M, D, A, S3, prec, kernel), x, BLOCKS)
        worst = spectrum_errors(got, ref)
        print(f"d M={M} K={K} D={D} A={A} {name(prec)} kernel={kernel}: worst spectrum {worst:.3e} (limit {TOL[prec]:.0e})")
        assert worst <= TOL[prec]


# ================================================================ e. closed forms at complex64
@gpu
@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("A", [5, 100])
@pytest.mark.parametrize("M,D", [(64, 64), (64, 32), (1024, 1024), (1024, 512)])
def test_dc(M, D, A, kernel):
    """amplitude 0.5 through an all-ones window of M points: P is exactly A M^2 / 4 at bin 0 and exactly 0
    elsewhere; at D < M the first spectrum sees the zero history and is held to the definition instead"""
    h, x = np.ones(M, F32), np.full((S3, FRAMES * D), 0.5, C64)
    P = run_blocks(tuned(h, M, D, A, S3, C64, kernel), x, BLOCKS)
    first = 0 if D == M else 1
    assert np.all(P[:, first:, 0] == A * M * M / 4) and not P[:, first:, 1:].any()
    if first:
        ref = spec_ref(h, M, D, A, x[0])
        assert spectrum_errors(P[:, 0], np.broadcast_to(ref[0], (S3, M))) <= TOL[C64]


@gpu
@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("A", [5, 100])
def test_tone_and_parseval(A, kernel):
    """M = 64, D = M, an all-ones window.  A tone a e^{-j 2 pi 5 (n+1) / M} lands on bin 5 (channel k mixes
    with e^{+j 2 pi k (n+1) / M}): the peak within tol of A M^2 |a|^2, every other bin below tol times
    the peak.  White input: sum_k P_j[k] within tol of M sum |x|^2 over the integration's samples"""
    M, tol = 64, TOL[C64]
    h = np.ones(M, F32)
    a, n = 0.75 - 0.5j, np.arange(FRAMES * M)
    tone = (a * np.exp(-2j * np.pi * ((5 * (n + 1)) % M) / M)).astype(C64)
    P = run_blocks(tuned(h, M, M, A, 1, C64, kernel), tone[None, :], BLOCKS)[0].astype(F64)
    peak = A * M * M * abs(a) ** 2
    assert np.all(np.abs(P[:, 5] - peak) <= tol * peak)
    rest = np.delete(P, 5, axis=1)
    print(f"e tone A={A} kernel={kernel}: largest other bin {rest.max() / peak:.3e} of the peak (limit {tol:.0e})")
    assert rest.max() <= tol * peak
    x = white_streams(S3, FRAMES * M)
    P = run_blocks(tuned(h, M, M, A, S3, C64, kernel), x, BLOCKS).astype(F64)
    J = FRAMES // A
    energy = (np.abs(x.astype(C128)) ** 2)[:, :J * A * M].reshape(S3, J, A * M).sum(axis=2) * M
    assert np.all(np.abs(P.sum(axis=2) - energy) <= tol * energy)


# ================================================================ f. scale
@gpu
@pytest.mark.parametrize("prec", [C64, C128], ids=["c64", "c128"])
@pytest.mark.parametrize("kernel", [1, 2])
def test_scale(kernel, prec):
    """set_scale between two calls: spectra completed afterwards are the unscaled run's times T(s), bit
    for bit, earlier ones untouched; the scale survives reset"""
    M, K, D, A = 64, 3, 48, 5
    T = coef_dtype(prec)
    h, x = white_input(M, K, D, prec)
    plain = run_blocks(tuned(h, M, D, A, S3, prec, kernel), x, BLOCKS)
    cut = sum(BLOCKS[:4])  # 45 frames: nine spectra before the change
    for s in (1.0 / (A * M), 0.1):
        sp = tuned(h, M, D, A, S3, prec, kernel)
        first = run_blocks(sp, x[:, :cut * D], BLOCKS[:4])
        sp.set_scale(s)
        ends = [int(e) for e in np.cumsum(BLOCKS)]
        rest = np.concatenate([call(sp, x[:, a * D:b * D], a) for a, b in zip(ends[3:-1], ends[4:])], axis=1)
        assert bits_equal(first, plain[:, :cut // A])
        assert bits_equal(rest, plain[:, cut // A:] * T(s))
        sp.reset()
        assert bits_equal(run_blocks(sp, x, BLOCKS), plain * T(s))


# ================================================================ g. state and calls
SMALL = (64, 4, 48, 33)  # M, K, D, A


@gpu
@pytest.mark.parametrize("kernel", [1, 2])
def test_reset_and_set_streams_zero_the_state(kernel):
    M, K, D, A = SMALL
    h, x = white_taps(M * K), white_streams(2, 100 * D)
    fresh = tuned(h, M, D, A, 2, C64, kernel, 1).execute_block(x[:, 41 * D:])
    assert fresh.shape == (2, 1, M)
    assert not bits_equal(fresh, tuned(h, M, D, A, 2, C64, kernel, 1).execute_block(x)[:, 1:2])  # the state matters
    sp = tuned(h, M, D, A, 2, C64, kernel, 1)
    assert sp.execute_block(x[:, :41 * D]).shape == (2, 1, M)
    assert (sp.filled, sp.phase) == (8, (41 * D) % M) and sp.phase != 0
    sp.reset()
    assert (sp.filled, sp.phase) == (0, 0)
    assert bits_equal(sp.execute_block(x[:, 41 * D:]), fresh)
    sp.set_streams(1)
    assert (sp.filled, sp.phase) == (0, 0)
    sp.execute_block(x[0, :35 * D])
    assert (sp.filled, sp.phase) == (2, (35 * D) % M)
    sp.set_streams(2)
    assert (sp.filled, sp.phase) == (0, 0)
    assert bits_equal(sp.execute_block(x[:, 41 * D:]), fresh)


@gpu
@pytest.mark.parametrize("kernel", [1, 2])
def test_streams_hosts_and_offsets(kernel):
    """three streams equal three one-stream handles; the host entry point equals the device path; input
    and output one sample past a 16-byte boundary give the same bits"""
    M, K, D, A = SMALL
    h, x = white_input(M, K, D)
    base = run_blocks(tuned(h, M, D, A, S3, C64, kernel, 1), x, BLOCKS)
    for s in range(S3):
        assert bits_equal(run_blocks(tuned(h, M, D, A, 1, C64, kernel, 1), x[s:s + 1], BLOCKS)[0], base[s]), s
    sp, one = tuned(h, M, D, A, S3, C64, kernel, 1), tuned(h, M, D, A, 1, C64, kernel, 1)
    cuts = np.cumsum([0] + BLOCKS) * D
    host = np.concatenate([sp.execute_block(x[:, a:b]) for a, b in zip(cuts[:-1], cuts[1:])], axis=1)
    assert host.dtype == F32 and bits_equal(host, base)
    host0 = np.concatenate([one.execute_block(x[0, a:b]) for a, b in zip(cuts[:-1], cuts[1:])])
    assert host0.shape == (FRAMES // A, M) and bits_equal(host0, base[0])
    assert bits_equal(run_blocks(tuned(h, M, D, A, S3, C64, kernel, 1), x, BLOCKS, in_off=1, out_off=1), base)


@gpu
@pytest.mark.parametrize("kernel", [1, 2])
def test_refused_calls_leave_the_state_untouched(kernel):
    """n % D != 0 and overlapping input and output are refused with SDSP_E_INVALID_ARGUMENT; filled and
    phase stay, and the next valid call equals an undisturbed handle's, bit for bit.  n = 0 emits nothing
    and changes nothing"""
    import torch
    M, K, D, A = SMALL
    h, x = white_input(M, K, D)
    calm, poked = tuned(h, M, D, A, S3, C64, kernel, 1), tuned(h, M, D, A, S3, C64, kernel, 1)
    assert bits_equal(call(calm, x[:, :41 * D], 0), call(poked, x[:, :41 * D], 0))
    state = (8, (41 * D) % M)
    st = torch.cuda.current_stream()
    n = 59 * D
    buf = empty_dev(S3 * n, C64)
    buf.copy_(to_dev(np.ascontiguousarray(x[:, 41 * D:100 * D]).reshape(-1)))
    d_out = empty_dev(S3 * 2 * M, F32)
    for bad in (D + 1, D - 1, 58 * D - 3):
        with pytest.raises(sd.SdspError) as e:
            poked.execute_block_device(buf, bad, d_out, st)
        assert e.value.code == E_INVALID_ARGUMENT and "whole number" in str(e.value)
        assert (poked.filled, poked.phase) == state
    reals = buf.view(torch.float32)
    for out in (reals, reals[2 * D:]):  # the same block; a block that starts inside the input
        with pytest.raises(sd.SdspError) as e:
            poked.execute_block_device(buf, n, out, st)
        assert e.value.code == E_INVALID_ARGUMENT and "overlap" in str(e.value)
        assert (poked.filled, poked.phase) == state
    assert sd.lib().sdsp_spec_execute_block(poked._h, None, D + 1, None, None) == E_INVALID_ARGUMENT
    assert poked.execute_block_device(buf, 0, d_out, st) == 0
    assert (poked.filled, poked.phase) == state
    assert bits_equal(call(calm, x[:, 41 * D:100 * D], 41), call(poked, x[:, 41 * D:100 * D], 41))


@gpu
def test_two_handles_alternate_on_two_streams():
    """two handles, each fed alternately from two torch streams: every call is ordered after the
    handle's last one, whichever stream that went to"""
    import torch
    M, K, D, A = SMALL
    h, x = white_input(M, K, D)
    base = run_blocks(tuned(h, M, D, A, S3, C64, 2, 1), x, BLOCKS)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    handles = [tuned(h, M, D, A, S3, C64, 1, 1), tuned(h, M, D, A, S3, C64, 2, 3)]
    torch.cuda.synchronize()
    outs, a = [[], []], 0
    for i, nb in enumerate(BLOCKS):
        for j, sp in enumerate(handles):
            outs[j].append(call(sp, x[:, a * D:(a + nb) * D], a, stream=streams[(i + j) % 2]))
        a += nb
    for j in range(2):
        assert bits_equal(np.concatenate(outs[j], axis=1), base), j


@gpu
def test_automatic_choice_is_the_restated_plan():
    """a handle as it comes reports spec_plan's kernel and sub-blocks at every shape of (a) and at the
    shapes behind the rule (tools/spec_ab.py); both kernels are chosen somewhere"""
    measured = [(M, K, D, A, C64) for M, D in ((64, 32), (64, 64), (128, 64), (256, 128), (1024, 512), (1024, 1024))
                for K in (1, 8) for A in (32, 1024)]
    chosen = set()
    for M, K, D, A, prec in SHAPES + measured:
        sp = sd.Spectrometer(white_taps(taps_len(M, K), prec), M, D, A, sample_dtype=prec)
        assert sp.info() == spec_plan(M, K, D, A, prec), (M, K, D, A, name(prec))
        chosen.add(sp.info()[0])
    assert chosen == {1, 2}


@gpu
def test_tuning_knobs():
    h = white_taps(1024 * 5)
    sp = sd.Spectrometer(h, 1024, 768, 100)
    assert sp.info() == spec_plan(1024, 5, 768, 100, C64) == (1, 1)
    sp.set_tuning(TUNE_KERNEL, 2)
    assert sp.info() == spec_plan(1024, 5, 768, 100, C64, 2)
    sp.set_tuning(TUNE_SUBBLOCKS, 7)
    assert sp.info() == (2, 7)
    sp.set_tuning(TUNE_KERNEL, 1)
    assert sp.info() == (1, 7)
    for key, v in ((TUNE_KERNEL, 3), (TUNE_KERNEL, -1), (TUNE_SUBBLOCKS, -1), (27, 1), (28, 1)):
        with pytest.raises(sd.SdspError) as e:
            sp.set_tuning(key, v)
        assert e.value.code == E_INVALID_ARGUMENT
    ch = sd.OversampledChannelizer(h, 1024, 768)
    for key in (TUNE_KERNEL, TUNE_SUBBLOCKS):  # other handles refuse the new knobs
        with pytest.raises(sd.SdspError) as e:
            ch.set_tuning(key, 1)
        assert e.value.code == E_INVALID_ARGUMENT
