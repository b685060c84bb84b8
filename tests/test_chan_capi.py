"""The channeliser's C-ABI boundary (sdsp_chan_*, include/sdsp.h) on the path it shares with
sdsp_ichan and sdsp_oschan: create refuses bad arguments in the family's one order (a null taps pointer
among them) and a missing device before any device work, every entry point refuses a null handle, and
on the GPU a refused block, reset and set_streams leave the state the siblings' tests pin for them
(test_gpu_ichan.py, test_gpu_oschan.py).  The GPU cases compare two handles bit for bit, as those do."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from gpu_util import bits_equal, empty_dev, to_dev, to_host

gpu = pytest.mark.gpu

E_COEFFICIENTS_LENGTH_ZERO, E_NOT_ENOUGH_FILTERS = 1, 4
E_INVALID_ARGUMENT, E_UNSUPPORTED, E_NO_DEVICE = 90, 91, 101
C64, C128 = np.complex64, np.complex128


def _create(lib, dtype, len_, M, device=0, null_taps=False, coef_dt=np.float32):
    taps = np.ones(max(len_, 1), dtype=coef_dt)
    h = C.c_void_p(0xdead)  # create must null it on every failure
    p = None if null_taps else taps.ctypes.data_as(C.c_void_p)
    rc = lib.sdsp_chan_create(C.byref(h), dtype, p, len_, M, device)
    return rc, h


def _message(lib):
    m = lib.sdsp_last_error()
    return m.decode() if isinstance(m, bytes) else (m or "")


def test_create_refuses_bad_arguments_in_order():
    """every argument check comes before the device check, so this holds with and without a GPU; each
    call breaks one more rule than the check it expects to fire, so the order shows"""
    import solid_dsp_amd as sd
    lib = sd.lib()
    # 1. null out (with everything else wrong too)
    assert lib.sdsp_chan_create(None, -1, None, 16, 0, 0) == E_INVALID_ARGUMENT
    for dtype in (-1, sd.RR32, sd.CC32, sd.RR64, sd.CC64, 6):  # 2. dtype, ahead of null taps and channels = 0
        rc, h = _create(lib, dtype, 16, 0, null_taps=True)
        assert rc == E_UNSUPPORTED and not h.value, dtype
        assert "SDSP_RC32" in _message(lib)
    rc, h = _create(lib, sd.RC32, 16, 0, null_taps=True)  # 3. null taps with len > 0, ahead of channels = 0
    assert rc == E_INVALID_ARGUMENT and not h.value
    assert "taps pointer is null" in _message(lib)
    rc, h = _create(lib, sd.RC32, 0, 0)  # 4. channels = 0, ahead of len = 0
    assert rc == E_NOT_ENOUGH_FILTERS and not h.value
    assert "NotEnoughFilters" in _message(lib)
    rc, h = _create(lib, sd.RC64, 0, 3, null_taps=True, coef_dt=np.float64)  # 5. len = 0 (null taps are fine then),
    assert rc == E_COEFFICIENTS_LENGTH_ZERO and not h.value                  # ahead of channels = 3
    assert "CoefficientsLengthZero" in _message(lib)
    for M in (1, 2, 3, 12, 1000, 8192, 1 << 20):  # 6. not a power of two in [4, 4096], ahead of len < channels
        rc, h = _create(lib, sd.RC32, 1, M)
        assert rc == E_UNSUPPORTED and not h.value, M
        assert "power of two" in _message(lib)
    for M, n in ((4, 3), (64, 63), (4096, 4095)):  # 7. len < channels
        rc, h = _create(lib, sd.RC32, n, M)
        assert rc == E_INVALID_ARGUMENT and not h.value, (M, n)
        assert "fewer taps" in _message(lib)


def test_no_device_fails_loudly():
    import solid_dsp_amd as sd
    lib = sd.lib()
    if sd.device_count() > 0:
        rc, h = _create(lib, sd.RC32, 16, 8, device=sd.device_count() + 7)
    else:
        rc, h = _create(lib, sd.RC32, 16, 8)
        with pytest.raises(sd.SdspError) as e:
            sd.Channelizer(np.ones(16, dtype=np.float32), 8)
        assert e.value.code == E_NO_DEVICE
    assert rc == E_NO_DEVICE and not h.value  # no CPU fallback


def test_null_handle_calls():
    import solid_dsp_amd as sd
    lib = sd.lib()
    sz = C.c_size_t(77)
    for call in (lambda: lib.sdsp_chan_reset(None), lambda: lib.sdsp_chan_set_streams(None, 2),
                 lambda: lib.sdsp_chan_set_tuning(None, 8, 1), lambda: lib.sdsp_chan_set_tuning(None, 9, 8),
                 lambda: lib.sdsp_chan_set_tuning(None, 15, 0), lambda: lib.sdsp_chan_synchronize(None),
                 lambda: lib.sdsp_chan_execute_block(None, None, 0, None, C.byref(sz)),
                 lambda: lib.sdsp_chan_execute_block_device(None, None, 0, None, C.byref(sz), None)):
        assert call() == E_INVALID_ARGUMENT
    assert sz.value == 77  # nothing written through a refused call's pointers
    lib.sdsp_chan_destroy(None)  # a no-op


# ---------------------------------------------------------------- GPU: M = 8, K = 3, two streams
M, K, S = 8, 3, 2


def _case(prec, frames):
    """(white taps with a tail the handle ignores, [S, frames M] white streams) in the precision"""
    h = np.random.default_rng(20261022).standard_normal(M * K + 3).astype(np.float32 if prec == C64 else np.float64)
    x = np.stack([O.synth(20261023, s, 0, M * frames, complex_=True) for s in range(S)]).astype(prec)
    return h, x


@gpu
@pytest.mark.parametrize("prec", [C64, C128], ids=["c64", "c128"])
def test_refused_blocks_leave_the_state_untouched(prec):
    """n % M != 0 and overlapping input and output are refused with SDSP_E_INVALID_ARGUMENT; the next valid
    block equals an undisturbed handle's continuation, bit for bit.  n = 0 returns 0 frames and changes
    nothing"""
    import torch
    import solid_dsp_amd as sd
    h, x = _case(prec, 9)
    st = torch.cuda.current_stream()

    def call(ch, a, b):
        d_in = to_dev(np.ascontiguousarray(x[:, a * M:b * M]).reshape(-1))
        d_out = empty_dev(S * (b - a) * M, prec)
        assert ch.execute_block_device(d_in, (b - a) * M, d_out, st) == b - a
        return to_host(d_out)

    calm = sd.Channelizer(h, M, sample_dtype=prec, streams=S)
    poked = sd.Channelizer(h, M, sample_dtype=prec, streams=S)
    assert bits_equal(call(calm, 0, 4), call(poked, 0, 4))
    d_in, d_out = to_dev(np.ascontiguousarray(x[:, 4 * M:]).reshape(-1)), empty_dev(S * 5 * M, prec)
    for n in (M + 1, M - 1, 5 * M - 3):
        with pytest.raises(sd.SdspError) as e:
            poked.execute_block_device(d_in, n, d_out, st)
        assert e.value.code == E_INVALID_ARGUMENT and "whole number" in str(e.value)
    for out in (d_in, d_in[M:]):  # the same block; a block that starts inside the input
        with pytest.raises(sd.SdspError) as e:
            poked.execute_block_device(d_in, 2 * M, out, st)
        assert e.value.code == E_INVALID_ARGUMENT and "overlap" in str(e.value)
    # the host entry point refuses a ragged n before it reads the block
    assert sd.lib().sdsp_chan_execute_block(poked._h, None, M + 1, None, None) == E_INVALID_ARGUMENT
    assert poked.execute_block_device(d_in, 0, d_out, st) == 0
    late = call(calm, 4, 9)
    assert bits_equal(late, call(poked, 4, 9))
    # (the history matters at these frames: a fresh handle gives other bits)
    assert not bits_equal(late, call(sd.Channelizer(h, M, sample_dtype=prec, streams=S), 4, 9))


@gpu
@pytest.mark.parametrize("prec", [C64, C128], ids=["c64", "c128"])
def test_reset_and_set_streams_zero_the_history(prec):
    import solid_dsp_amd as sd
    h, x = _case(prec, 6)
    cut = 3 * M
    fresh = sd.Channelizer(h, M, sample_dtype=prec, streams=S).execute_block(x[:, cut:])
    whole = sd.Channelizer(h, M, sample_dtype=prec, streams=S).execute_block(x)
    assert not bits_equal(fresh, whole[:, 3:])  # the history matters
    ch = sd.Channelizer(h, M, sample_dtype=prec, streams=S)
    ch.execute_block(x[:, :cut])
    ch.reset()
    assert bits_equal(ch.execute_block(x[:, cut:]), fresh)
    ch.set_streams(1)
    ch.execute_block(x[0, :cut])
    ch.set_streams(S)
    assert bits_equal(ch.execute_block(x[:, cut:]), fresh)
