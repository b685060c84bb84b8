"""Rational resampler on MI355X: an M/D polyphase FIR that computes only the outputs it keeps.

A build-defined composition of reference objects (src/filter/fir/interp.rs,
src/filter/fir/decim.rs), as the channeliser and the two converters are:
``Resampler(taps, M, D)`` with phase counter ``c`` (interpolated samples since the
last one kept, 0 after construction and ``reset``) writes, for a block of ``n``
inputs per channel,

    z = interpolator.execute_block(x)                       # n * M samples
    out[k] = z[(k + 1) * D - 1 - c],  k < n_out = (c + n * M) // D
    c = (c + n * M) % D

in one pass (``kern_resamp.hip``): the interpolated stream is never written and the
D - 1 of every D dot products a caller would discard are never computed.
``ALGO_EXACT`` is bit-identical to an ``ALGO_EXACT`` ``InterpolatingFIRFilter``
whose output is taken at ``[D - 1 - c :: D]``; ``ALGO_FMA`` sums with fused
multiply-adds.  Any of the six (taps, sample) pairs.  There is no scale (the
interpolator has none).  A block object: there is no per-sample ``execute``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _handle as H
from . import _lib as L


def count(interpolation: int, decimation: int, phase: int, n: int):
    """(n_out, next_phase) of a block of n inputs: sdsp_resamp_count, no handle and no device"""
    n_out, nxt = C.c_size_t(), C.c_size_t()
    L.check(L.lib().sdsp_resamp_count(interpolation, decimation, phase, n, C.byref(n_out), C.byref(nxt)))
    return n_out.value, nxt.value


class Resampler(H.FirHandle):
    _family = "resamp"
    KERNELS = {1: "staged", 2: "per_output", 3: "branch"}

    def __init__(self, taps, interpolation=1, decimation=1, sample_dtype=None, coef_dtype=None, device=0, channels=1,
                 algo=None):
        c = self._coefs(taps, sample_dtype, coef_dtype)
        h = C.c_void_p()
        L.check(L.lib().sdsp_resamp_create(C.byref(h), self.dtype, L.ptr(c), len(c), int(interpolation),
                                           int(decimation), int(device)))
        self._adopt(h, device, channels, algo)  # algo None: ALGO_FMA when the process default is, else ALGO_EXACT

    @classmethod
    def new(cls, taps, interpolation, decimation, **kw):
        return cls(taps, interpolation, decimation, **kw)

    # ---- configuration -------------------------------------------------
    set_channels = H.set_channels  # zeroes the windows and the phase
    set_algo, get_algo = H.set_algo, H.get_algo  # ALGO_EXACT or ALGO_FMA
    set_tuning = H.set_tuning  # TUNE_RESAMP_KERNEL: 0 automatic, 1 staged, 2 per output, 3 branch-stationary

    def interpolation(self) -> int:
        return int(L.lib().sdsp_resamp_interpolation(self._h))

    def decimation(self) -> int:
        return int(L.lib().sdsp_resamp_decimation(self._h))

    def subfilter_len(self) -> int:
        return int(L.lib().sdsp_resamp_subfilter_len(self._h))

    def phase(self) -> int:
        p = C.c_size_t()
        L.check(L.lib().sdsp_resamp_get_phase(self._h, C.byref(p)))
        return p.value

    def set_phase(self, phase: int):
        L.check(L.lib().sdsp_resamp_set_phase(self._h, int(phase)))

    def output_count(self, n: int) -> int:
        """outputs per channel a block of n inputs produces from the current phase"""
        return int(L.lib().sdsp_resamp_output_count(self._h, n))

    def info(self):
        """(kernel, tile): the kernel the next call runs (1 staged, 2 per output, 3
        branch-stationary) and its outputs per workgroup"""
        k, t = C.c_int(), C.c_size_t()
        L.check(L.lib().sdsp_resamp_info(self._h, C.byref(k), C.byref(t)))
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
            L.check(L.lib().sdsp_resamp_execute_block(self._h, L.ptr(x), n, L.ptr(y), C.byref(got)))
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
        L.check(L.lib().sdsp_resamp_execute_block_device(self._h, pin, n, pout, C.byref(got),
                                                         L.stream_handle(stream)))
        return got.value
