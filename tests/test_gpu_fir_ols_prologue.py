"""The one-shot overlap-save kernel's segment arithmetic at the shapes where it can go wrong:
the interior launch deals workgroup b to segment lo + (b % 8) q + b / 8 with q = ceil(count / 8)
and refuses seg >= hi, all in 32 bits on the scalar unit, and adds the channel's offset to the
segment's.  Block lengths give the interior launch 0, 1, 7, 8, 9 and 17 segments (no launch, empty
eighths, one segment per XCD, ragged eighths), with one halo row compiled in (L = 256) and the
generic instance (L = 700, three halo rows), 8-byte and 16-byte lanes, 1 and 3 channels.

The rule, restated: V = 4096 - 256 h2 outputs per segment, segment s reads the window
[s V - 256 h2, s V - 256 h2 + 4096) of its block; it is interior when that window lies inside the
block and it is not the block's last segment (which runs in the boundary launch and writes the
next history)."""
import functools

import numpy as np
import pytest

import oracle_lib as O
from gpu_util import bits_equal, rel_rms

pytestmark = pytest.mark.gpu

sd = pytest.importorskip("solid_dsp_amd")
from solid_dsp_amd import FIRFilter  # noqa: E402

C64, C128, F32 = np.complex64, np.complex128, np.float32
TUNE_OLS_KERNEL = 14
OLS_ONESHOT, OLS_ONESHOT_WIDE = 0, 3
CH = 3
HEAD = 778   # a first, short block: the main block then starts from a history that is not zero
TAIL = 1234  # samples past a whole number of segments (even: 3 channels of odd length take the scalar kernel)


def interior_segments(n, L):
    h2 = -(-(L - 1) // 256)
    V, H = 4096 - 256 * h2, 256 * h2
    nseg = -(-n // V)
    return sum(1 for s in range(nseg) if s * V - H >= 0 and s * V - H + 4096 <= n and s != nseg - 1)


def block_length(L, k):
    """a block with k interior segments: k + 1 whole advances and a ragged tail"""
    h2 = -(-(L - 1) // 256)
    return (k + 1) * (4096 - 256 * h2) + TAIL


def taps(L):
    h = O.firdes_kaiser(L, 0.1, 80.0, 0.0).astype(F32)
    return (h * np.exp(2j * np.pi * 0.05 * np.arange(L))).astype(C64)


@functools.lru_cache(maxsize=None)
def case(L, k):
    """(inputs [CH][HEAD + n], f64 restatement of every channel), shared by both kernels"""
    n = block_length(L, k)
    x = O.synth(20250231, 3, 0, CH * (HEAD + n), complex_=True).reshape(CH, -1)
    h = taps(L)
    ref = np.stack([O.fir(O.CC64, h.astype(C128), 0.2 + 0j).execute_block(x[c].astype(C128)) for c in range(CH)])
    x.setflags(write=False)
    ref.setflags(write=False)
    return x, ref


def run(L, kern, x):
    """the short block, then the main one; (outputs, state after)"""
    ch = x.shape[0] if x.ndim > 1 else 1
    f = FIRFilter(taps(L), C64(0.2), sample_dtype=C64, channels=ch, algo=sd.ALGO_FFT, host_step=False)
    assert sd.lib().sdsp_fir_set_tuning(f._h, TUNE_OLS_KERNEL, kern) == 0
    y = np.concatenate([f.execute_block(x[..., :HEAD]), f.execute_block(x[..., HEAD:])], axis=-1)
    hist, _ = f.get_state()
    return y, hist


@pytest.mark.parametrize("k", [0, 1, 7, 8, 9, 17])
@pytest.mark.parametrize("kern", [OLS_ONESHOT, OLS_ONESHOT_WIDE])
@pytest.mark.parametrize("L", [256, 700])
def test_oneshot_interior_segment_counts(L, kern, k):
    n = block_length(L, k)
    assert n < 80000 and n % 2 == 0 and interior_segments(n, L) == k
    x, ref = case(L, k)
    h = taps(L)
    y3, hist3 = run(L, kern, x)
    assert bits_equal(hist3, x[:, -(L - 1):].reshape(-1))
    for c in range(CH):
        y1, hist1 = run(L, kern, x[c])
        assert bits_equal(hist1, x[c, -(L - 1):]), (L, kern, k, c)
        r, worst = rel_rms(y1, ref[c]), np.abs(y1 - ref[c]).max()
        bound = 1e-6 * np.abs(h).sum() * 0.2 * np.abs(x[c]).max()
        print(f"L={L} kern={kern} interior={k} ch={c}: rel_rms {r:.3e} max|err| {worst:.3e} (bound {bound:.3e})")
        assert r <= 1e-6, (L, kern, k, c)
        assert worst <= bound, (L, kern, k, c)
        assert rel_rms(y3[c], ref[c]) <= 1e-6 and np.abs(y3[c] - ref[c]).max() <= bound, (L, kern, k, c)
        # the 3-channel call is three 1-channel calls
        assert bits_equal(y3[c], y1), (L, kern, k, c)
