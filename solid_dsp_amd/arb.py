"""Arbitrary-rate resampler on MI355X: any rate from one polyphase bank.

A build-defined composition on the reference's ``PolyPhaseFilterBank``
(src/filter/fir/pfb.rs: ``push``, then ``execute(index)`` with a caller-chosen
branch): ``ArbResampler(taps, P, rate=r)`` keeps a Q32.32 time accumulator ``t``
(time of the next output from the first input of the next call, 0 after
construction and ``reset``) and a Q32.32 ``step`` of input samples per output
(``step = round(2**32 / rate)``).  With ``z`` the ``ALGO_EXACT``
``InterpolatingFIRFilter(taps, P)`` stream over the whole input history, a block of
``n`` inputs per channel writes

    T = t + k * step;  j = T >> 32;  f = T & (2**32 - 1)
    v = f * P;  b = v >> 32;  mu = (v & (2**32 - 1)) * 2**-32
    u = j * P + b
    out[k] = z[u - 1] + mu * (z[u] - z[u - 1]),  k < n_out = ceil((n * 2**32 - t) / step)
    t = t + n_out * step - n * 2**32

in one pass (``kern_arb.hip``): the interpolated stream is never written and no
look-ahead is needed (the handle delays by 1 / P of an input sample relative to
interpolating between ``z[u]`` and ``z[u + 1]``).  ``ALGO_EXACT`` is bit-identical to
that formula applied to the ``ALGO_EXACT`` interpolator's output in the sample
dtype; ``ALGO_FMA`` sums with fused multiply-adds and ends with ``fma(mu, c - a, a)``.
Any of the six (taps, sample) pairs.  There is no scale.  A block object: there is
no per-sample ``execute``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _handle as H
from . import _lib as L


def count(step: int, t: int, n: int):
    """(n_out, next_t) of a block of n inputs: sdsp_arb_count, no handle and no device"""
    n_out, nxt = C.c_size_t(), C.c_uint64()
    L.check(L.lib().sdsp_arb_count(step, t, n, C.byref(n_out), C.byref(nxt)))
    return n_out.value, nxt.value


def step_from_rate(rate: float) -> int:
    """the Q32.32 step of an output rate (outputs per input): sdsp_arb_step_from_rate"""
    step = C.c_uint64()
    L.check(L.lib().sdsp_arb_step_from_rate(float(rate), C.byref(step)))
    return step.value


class ArbResampler(H.FirHandle):
    _family = "arb"
    KERNELS = {1: "staged", 2: "per_output"}

    def __init__(self, taps, filters, rate=None, step=None, sample_dtype=None, coef_dtype=None, device=0, channels=1,
                 algo=None):
        if (rate is None) == (step is None):
            raise ValueError("exactly one of rate and step must be given")
        if step is None:
            step = step_from_rate(rate)
        c = self._coefs(taps, sample_dtype, coef_dtype)
        h = C.c_void_p()
        L.check(L.lib().sdsp_arb_create(C.byref(h), self.dtype, L.ptr(c), len(c), int(filters), int(step),
                                        int(device)))
        self._adopt(h, device, channels, algo)  # algo None: ALGO_FMA when the process default is, else ALGO_EXACT

    @classmethod
    def new(cls, taps, filters, **kw):
        return cls(taps, filters, **kw)

    # ---- configuration -------------------------------------------------
    set_channels = H.set_channels  # zeroes the windows and the time
    set_algo, get_algo = H.set_algo, H.get_algo  # ALGO_EXACT or ALGO_FMA
    set_tuning = H.set_tuning  # TUNE_ARB_KERNEL: 0 automatic, 1 staged, 2 per output

    def filters(self) -> int:
        return int(L.lib().sdsp_arb_filters(self._h))

    def subfilter_len(self) -> int:
        return int(L.lib().sdsp_arb_subfilter_len(self._h))

    def step(self) -> int:
        """input samples per output, Q32.32"""
        s = C.c_uint64()
        self._call("get_step", C.byref(s))
        return s.value

    def set_step(self, step: int):
        """takes effect at the next output; the time stays"""
        self._call("set_step", int(step))

    def rate(self) -> float:
        return float(2 ** 32) / self.step()

    def set_rate(self, rate: float):
        self.set_step(step_from_rate(rate))

    def time(self) -> int:
        """time of the next output from the first input of the next call, Q32.32"""
        t = C.c_uint64()
        self._call("get_time", C.byref(t))
        return t.value

    def set_time(self, t: int):
        self._call("set_time", int(t))

    def output_count(self, n: int) -> int:
        """outputs per channel a block of n inputs produces from the current step and time"""
        return int(L.lib().sdsp_arb_output_count(self._h, n))

    def info(self):
        """(kernel, tile): the kernel the next call runs (1 staged, 2 per output) and its
        outputs per workgroup"""
        k, t = C.c_int(), C.c_size_t()
        self._call("info", C.byref(k), C.byref(t))
        return k.value, t.value

    # ---- blocks ----------------------------------------------------------
    def execute_block(self, samples) -> np.ndarray:
        """Host samples (channel-major [channels, n] when channels > 1) -> [n_out] or
        [channels, n_out]."""
        x, n = self._block_in(samples)
        no = self.output_count(n)
        y = self._block_out(no)
        if n:
            got = C.c_size_t()
            L.check(L.lib().sdsp_arb_execute_block(self._h, L.ptr(x), n, L.ptr(y), C.byref(got)))
            assert got.value == no
        return y

    def execute_block_device(self, d_in, n: int, d_out, stream=None) -> int:
        """Device-resident block: d_in / d_out are torch tensors or raw device pointers
        (channel-major, n samples per channel in, output_count(n) per channel out).  Returns
        n_out."""
        no = self.output_count(n)
        pin = L.device_ptr(d_in, self.sample_dtype, self.channels * n, self.device, "input")
        pout = L.device_ptr(d_out, self.sample_dtype, self.channels * no, self.device, "output")
        got = C.c_size_t()
        L.check(L.lib().sdsp_arb_execute_block_device(self._h, pin, n, pout, C.byref(got), L.stream_handle(stream)))
        return got.value
