"""The receive chain's launch rules, restated, and the case tables built on them.

launch_acorr, launch_nco_mix and launch_agc (csrc/kern_rx.hip) choose a kernel, a grid and, inside
the kernels, a code shape from (W, d, n), from two pointers' alignment and from (n, channels).  None
of the three handles can say which path a call took, so the tests name it from this restatement:
every function below gives the lines of kern_rx.hip it restates, and a reader has to hold the two
side by side.  No GPU import: the CPU suite checks that the case tables reach every path and every
boundary (tests/test_rx_cases.py), the GPU suite runs them (tests/test_gpu_rx_paths.py).
"""
from __future__ import annotations

import math

import numpy as np

C64, C128 = np.complex64, np.complex128
DTYPES = (C64, C128)

# kern_rx.hip:45-48, :85, :216
K_TILE, K_R = 64, 8
K_OUT = K_TILE * K_R        # outputs per workgroup (one tile)
K_CHUNK = 256               # terms per pass of the one-shot kernel
K_DMAX = 256                # largest delay the one-shot kernel stages in LDS
K_PIPE_K = K_PIPE_D = 128   # limits of the pipelined kernel
# acorr_pipe_slots (:703-721) asks the device; any value >= a call's interior tiles launches alike,
# and every call below has at most 30 tiles
RESIDENT_DEFAULT = 256 * 8
TUNE_ACORR_KERNEL, TUNE_AGC_KERNEL, TUNE_ACORR_SLOTS = 20, 21, 30


# ---------------------------------------------------------------- AutoCorrelator: the rule
def acorr_k(W, d):
    """runtime_rx.cpp sdsp_acorr::K: product terms per output"""
    return max(W - d, 0)


PIPE_BRANCHES = ("K<8", "head-only", "m7-only", "scalar", "block", "both")


def pipe_sum_shape(K):
    """acorr_pipe_kernel's sum, kern_rx.hip:301-347, walked for one K: the head (K >= 8), the
    scalar body down to the next m & 7 == 7, blocks of eight while m >= 15, the lone m == 7 term,
    the tail.  Returns (branch name, scalar terms, blocks, lone)."""
    if K < K_R:
        return "K<8", 0, 0, False
    m, scalar, blocks = K - 2, 0, 0
    while m >= K_R - 1 and (m & 7) != 7:
        scalar, m = scalar + 1, m - 1
    while m >= 15:
        blocks, m = blocks + 1, m - 8
    lone = m == K_R - 1
    # every term m = K - 2 .. 7 is added exactly once
    assert scalar + 8 * blocks + (1 if lone else 0) == max(K - 2 - 6, 0), K
    if K == 8:
        name = "head-only"
    elif not scalar and not blocks:
        name = "m7-only"
    elif scalar and blocks:
        name = "both"
    else:
        name = "scalar" if scalar else "block"
    return name, scalar, blocks, lone


def oneshot_chunks(K):
    """acorr_kernel's chunk loop, kern_rx.hip:103-104 and :177-200: (cj, "cj>=8" | "edge") per chunk"""
    out = []
    for j0 in range(0, K, K_CHUNK):
        cj = min(K - j0, K_CHUNK)
        out.append((cj, "cj>=8" if cj >= K_R else "edge"))
    return out


def pipe_walk(t_lo, t_hi, G):
    """acorr_pipe_kernel's XCD-ordered walk, kern_rx.hip:237-241 and :271-365: workgroup b takes
    tiles e_lo + (b >> 3) + i Gx of eighth b & 7.  Returns (tiles per workgroup, tiles per eighth)."""
    nt = t_hi - t_lo
    Q, Gx = (nt + 7) // 8, G // 8
    walks, eighths = [], [0] * 8
    seen = []
    for b in range(G):
        e_lo = t_lo + (b & 7) * Q
        e_hi = min(e_lo + Q, t_hi)
        tiles = list(range(e_lo + (b >> 3), max(e_hi, e_lo + (b >> 3)), Gx)) if e_lo + (b >> 3) < e_hi else []
        walks.append(len(tiles))
        eighths[b & 7] += len(tiles)
        seen += tiles
    assert sorted(seen) == list(range(t_lo, t_hi)), (t_lo, t_hi, G)  # every interior tile once
    return walks, eighths


def acorr_plan(W, d, n, kernel=0, slots=0, resident=RESIDENT_DEFAULT):
    """launch_acorr, kern_rx.hip:723-783.  launches: (kernel, first tile, end tile) in launch order;
    kernel is "pipe", "oneshot-stage" (STAGE) or "oneshot-2load"."""
    K = acorr_k(W, d)
    ntiles = (n + K_OUT - 1) // K_OUT
    plan = {"K": K, "d": d, "n": n, "ntiles": ntiles, "pipe": None, "chunks": oneshot_chunks(K),
            "pipe_eligible": kernel == 0 and 1 <= K <= K_PIPE_K and d <= K_PIPE_D}
    if n == 0:
        plan.update(launches=[], stage=None)
        return plan
    if plan["pipe_eligible"]:
        t_lo, t_hi = (K - 1 + d + K_OUT - 1) // K_OUT, n // K_OUT
        plan["t_lo"], plan["t_hi"] = t_lo, t_hi
        if t_hi > t_lo:
            res = resident
            if 0 < slots < res:
                res = slots
            nt = t_hi - t_lo
            G = (min(nt, res) + 7) // 8 * 8
            walks, eighths = pipe_walk(t_lo, t_hi, G)
            launches = [("pipe", t_lo, t_hi)]
            for a, b in ((0, t_lo), (t_hi, ntiles)):
                if b > a:
                    launches.append(("oneshot-stage", a, b))
            plan.update(launches=launches, stage=True, pipe={
                "G": G, "Q": (nt + 7) // 8, "walks": walks, "eighths": eighths,
                "branch": pipe_sum_shape(K)[0], "leading": t_lo, "trailing": ntiles - t_hi})
            return plan
    stage = d <= K_DMAX and kernel != 2
    plan.update(launches=[("oneshot-stage" if stage else "oneshot-2load", 0, ntiles)], stage=stage)
    return plan


# ---------------------------------------------------------------- AutoCorrelator: the cases
# every entry: (W, d, calls, kernel knob, slots knob, channels); one handle runs `calls` in order
N_BRANCH = (4 * K_OUT + 77, 3 * K_OUT)   # edge tile on history + 3 interior + ragged tile; whole tiles
N_ONESHOT = (2 * K_OUT + 77, 300)
N_SLOTS = (30 * K_OUT + 77, 12 * K_OUT + 1)
N_CHANNELS = (1, 7, 40, 1100)

BRANCH_K = (1, 2, 7, 8, 9, 10, 15, 16, 17, 18, 23, 24, 25, 31, 32, 33, 127, 128)
BRANCH_K += (11, 12, 13, 14, 19, 20, 21, 22)  # the other residues of K mod 8, without and with a block
DELAYS = (0, 1, 127, 128, 129, 255, 256, 257)
ONESHOT_K = (129, 255, 256, 257, 259, 263, 264, 512, 513, 700)
ONESHOT_D = (0, 5, 300)
KNOB_K = {1: (1, 3, 7, 8, 48, 128), 2: (3, 48, 300)}
SLOTS_K, SLOTS_D = (5, 9, 17, 48, 128), (0, 16, 128)

ACORR_BRANCH = [(K + 3, 3, N_BRANCH, 0, 0, 1) for K in BRANCH_K]
ACORR_DELAY = [(16 + d, d, N_BRANCH, 0, 0, 1) for d in DELAYS] + [(256, 128, N_BRANCH, 0, 0, 1)]
ACORR_NO_INTERIOR = [(8, 3, (600,), 0, 0, 1)]
ACORR_ONESHOT = [(K + d, d, N_ONESHOT, 0, 0, 1) for d in ONESHOT_D for K in ONESHOT_K]
ACORR_KNOB = [(K + 16, 16, N_BRANCH, knob, 0, 1) for knob, ks in KNOB_K.items() for K in ks]
ACORR_SLOTS = [(K + d, d, (n,), 0, 1, 2) for n in N_SLOTS for d in SLOTS_D for K in SLOTS_K]
ACORR_CHANNELS = [(48, 16, N_CHANNELS, 0, 0, 3), (300, 5, N_CHANNELS, 0, 0, 3)]
ACORR_ALL = (ACORR_BRANCH + ACORR_DELAY + ACORR_NO_INTERIOR + ACORR_ONESHOT + ACORR_KNOB + ACORR_SLOTS
             + ACORR_CHANNELS)

K_BOUNDARIES = (1, 7, 8, 9, 15, 16, 17, 127, 128, 129, 255, 256, 257, 263, 264, 512, 513)
D_BOUNDARIES = (0, 1, 127, 128, 129, 255, 256, 257)


def acorr_id(case):
    W, d, calls, knob, slots, ch = case
    return f"W{W}-d{d}-n{calls[0]}-k{knob}-s{slots}-c{ch}"


def case_plans(case):
    """the plan of every call of a case"""
    W, d, calls, knob, slots, _ = case
    return [acorr_plan(W, d, n, knob, slots) for n in calls]


def crand(seed, shape, dt):
    """complex normal samples in the handle's precision"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(dt)


def acorr_input(case, dt):
    """[channels, sum(calls)] samples of a case (the same for both precisions, rounded to dt)"""
    W, d, calls, knob, slots, ch = case
    return crand(1000003 * W + 1009 * d + 17 * knob + slots + sum(calls), (ch, sum(calls)), dt)


# ---------------------------------------------------------------- NCO: the rule
NCO_U, NCO_THREADS = 8, 256
NCO_BLOCK_VECS = NCO_U * NCO_THREADS  # vectors per workgroup


def nco_plan(n, prec, in_aligned=True, out_aligned=True):
    """launch_nco_mix and nco_mix_kernel, kern_rx.hip:807-829 and :417-462: V samples per lane
    (2 for c32 through two 16-byte-aligned pointers), nv whole vectors, the tail lane's samples"""
    V = 2 if prec == 0 and in_aligned and out_aligned else 1
    nv = n // V
    blocks = max((nv + NCO_BLOCK_VECS - 1) // NCO_BLOCK_VECS, 1)
    last = nv - (blocks - 1) * NCO_BLOCK_VECS  # vectors of the last workgroup
    return {"V": V, "nv": nv, "blocks": blocks, "tail": n - nv * V, "last_block_vecs": last,
            "bounded_store": prec == 0 and V == 2}  # kWt: 16-byte vectors through a descriptor


def nco_form(n, prec, in_aligned=True, out_aligned=True):
    """what a call exercises, as a tuple the coverage test can collect"""
    p = nco_plan(n, prec, in_aligned, out_aligned)
    if p["nv"] == 0:
        fill = "empty"       # no vector at all: an empty store descriptor, the tail lane only
    elif p["last_block_vecs"] == NCO_BLOCK_VECS:
        fill = "full"        # the last workgroup has all its 2048 vectors
    elif p["last_block_vecs"] == 1 and p["blocks"] > 1:
        fill = "one-over"    # one vector spills into a further workgroup
    else:
        fill = "part"
    why = "v2" if p["V"] == 2 else ("c64" if prec == 1 else
                                    {(False, True): "in-off", (True, False): "out-off",
                                     (False, False): "both-off"}[(in_aligned, out_aligned)])
    return why, min(p["blocks"], 3), fill, p["tail"]


NCO_N = (1, 2, 3, 2047, 2048, 2049, 4095, 4096, 4097, 4099, 8193)
NCO_SHAPES = ((0, 0), (1, 0), (0, 1), (1, 1))  # (input, output) offset in samples from 16-byte alignment
NCO_PHASES = ((0xFFFFFF00, 0x9E3779B9), (0xFFE00000, 0), (0xFFDFFFFF, 1))
NCO_GUARD = 64  # sentinel samples on each side of the n written


def nco_table():
    """NCO::new's sine table (src/nco/mod.rs:36-50; runtime_rx.cpp nco_sine_table), through the C
    library's sin as both the handle and the restatement compute it"""
    return np.array([math.sin(2.0 * math.pi * float(i) / 1024.0) for i in range(1024)], dtype=np.float64)


def nco_index(theta):
    """idx = ((theta + 2^21) mod 2^32 >> 22) & 1023 (src/nco/mod.rs:99-101)"""
    return ((((np.asarray(theta, dtype=np.uint64) + np.uint64(1 << 21)) & np.uint64(0xFFFFFFFF))
             >> np.uint64(22)) & np.uint64(1023)).astype(np.int64)


def nco_thetas(theta0, dtheta, n):
    i = np.arange(n, dtype=np.uint64)
    return (np.uint64(theta0) + i * np.uint64(dtheta)) & np.uint64(0xFFFFFFFF)


def nco_model(x, theta0, dtheta, down, real_dtype):
    """The mixing kernel's arithmetic in NumPy at `real_dtype` (float32 for the c32 kernel): the
    table rounded to the type, the phasor (tab[(idx + 256) & 1023], +-tab[idx]), then mul_(ph, v)
    of sdsp_device.hpp with every product and sum rounded on its own (arrays of the type, nothing
    fused): re = c xr - s xi, im = c xi + s xr."""
    ft = np.dtype(real_dtype).type
    tab = nco_table().astype(ft)
    idx = nco_index(nco_thetas(theta0, dtheta, len(x)))
    c, s = tab[(idx + 256) & 1023], tab[idx]
    if down:
        s = -s
    xr, xi = np.ascontiguousarray(x.real, dtype=ft), np.ascontiguousarray(x.imag, dtype=ft)
    p0, p1, p2, p3 = c * xr, s * xi, c * xi, s * xr
    out = np.empty(len(x), dtype=np.complex64 if ft is np.float32 else np.complex128)
    out.real = p0 - p1
    out.imag = p2 + p3
    return out


def nco_end_state(theta0, dtheta, n):
    return (theta0 + n * dtheta) & 0xFFFFFFFF


# ---------------------------------------------------------------- AGC: the rule
AGC_S_PLAIN, AGC_S_PIPE, AGC_PIPE_MAX_N = 8, 16, 1 << 22
SQ_ENABLED, SQ_RISE, SQ_SIGNALHI, SQ_FALL, SQ_SIGNALLO, SQ_TIMEOUT, SQ_DISABLED = 1, 2, 3, 4, 5, 6, 7


def agc_plan(n, channels, knob=0, cplx=True):
    """launch_agc, kern_rx.hip:831-851; agc_pipe_kernel :596, :632, :652; agc_kernel :543-544"""
    pipe = knob == 0 and n < AGC_PIPE_MAX_N
    S = AGC_S_PIPE if pipe else AGC_S_PLAIN
    wgs = (channels + 63) // 64
    nfull = n // S * S
    return {"kernel": "pipe" if pipe else "plain", "S": S, "nfull": nfull, "ragged": n - nfull,
            "workgroups": wgs, "idle_lanes": wgs * 64 - channels, "sample_bytes": 16 if cplx else 8}


def agc_form(n, channels, knob, cplx):
    p = agc_plan(n, channels, knob, cplx)
    length = "nfull=0" if p["nfull"] == 0 else ("exact" if p["ragged"] == 0 else "whole+ragged")
    return p["kernel"], "complex" if cplx else "real", length


AGC_EDGE_CALLS = (1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 100)
AGC_EDGE_CHANNELS = 65
AGC_EDGE_EXTRA_CHANNELS = (1, 63, 64, 130)  # pipelined complex form only
AGC_HET_CHANNELS = 70
AGC_HET_PARTS = (100, 90, 61)   # burst, silence, burst
AGC_HET_CALLS = (57, 103, 91)   # 251 samples: ragged against 16 and against 8
AGC_INIT_N = (1, 5, 1000)
assert sum(AGC_HET_PARTS) == sum(AGC_HET_CALLS) and sum(AGC_HET_CALLS) % 16 and sum(AGC_HET_CALLS) % 8


def agc_edge_input(channels, cplx):
    """one stream for the chunk-edge calls: per-channel level over 1e-3 .. 1, a quiet stretch in
    the middle so the squelch (on, -30 dB) moves through its states"""
    n = sum(AGC_EDGE_CALLS)
    rng = np.random.default_rng(31 + channels + (1 if cplx else 0))
    amp = 10.0 ** rng.uniform(-3, 0, channels)
    x = rng.standard_normal((channels, n))
    if cplx:
        x = x + 1j * rng.standard_normal((channels, n))
    x = x * amp[:, None]
    x[:, 120:200] *= 1e-9
    return np.ascontiguousarray(x)


def agc_het_params(channels=AGC_HET_CHANNELS):
    """the heterogeneous bank: every channel its own loop bandwidth, scale, squelch switch,
    threshold and timeout; every seventh locked.  Strides coprime to each list's length, so the
    values combine differently from channel to channel."""
    out = []
    for c in range(channels):
        out.append({
            "bandwidth": 0.01 * 30.0 ** (((c * 37) % channels) / (channels - 1.0)),   # 0.01 .. 0.3
            "scale": (0.5, 1.0, 3.0)[c % 3],
            "squelch": c % 5 != 4,
            "threshold": -40.0 + 30.0 * ((c * 11) % channels) / (channels - 1.0),      # -40 .. -10
            "timeout": (1, 5, 37)[(c // 2) % 3],
            "lock": c % 7 == 6,
        })
    return out


def agc_het_input(cplx, channels=AGC_HET_CHANNELS):
    """burst, silence, burst per channel; burst levels spread over 1e-4 .. 10 (another level for
    the second burst), silence exactly zero on even channels and 1e-12 of the burst on odd ones"""
    rng = np.random.default_rng(41 + (1 if cplx else 0))
    n = sum(AGC_HET_PARTS)
    a, b = AGC_HET_PARTS[0], AGC_HET_PARTS[0] + AGC_HET_PARTS[1]
    x = rng.standard_normal((channels, n))
    if cplx:
        x = x + 1j * rng.standard_normal((channels, n))
    c = np.arange(channels)
    amp1 = 10.0 ** (-4.0 + 5.0 * ((c * 13) % channels) / (channels - 1.0))
    amp2 = 10.0 ** (-4.0 + 5.0 * ((c * 29 + 7) % channels) / (channels - 1.0))
    x[:, :a] *= amp1[:, None]
    x[:, a:b] *= np.where(c % 2 == 0, 0.0, 1e-12 * amp1)[:, None]
    x[:, b:] *= amp2[:, None]
    return np.ascontiguousarray(x)


def agc_init_input(n, cplx, channels=AGC_HET_CHANNELS):
    rng = np.random.default_rng(51 + n + (1 if cplx else 0))
    amp = 10.0 ** rng.uniform(-4, 1, channels)
    x = rng.standard_normal((channels, n))
    if cplx:
        x = x + 1j * rng.standard_normal((channels, n))
    return np.ascontiguousarray(x * amp[:, None])


def agc_oracle(O, p):
    """the restatement's AGC with one channel's parameters of agc_het_params"""
    o = O.Agc()
    assert o.set_bandwidth(p["bandwidth"]) == 0
    o.set_scale(p["scale"])
    o.squelch(1 if p["squelch"] else 0)
    o.squelch_set_threshold(p["threshold"])
    o.squelch_set_timeout(p["timeout"])
    o.lock(1 if p["lock"] else 0)
    return o
