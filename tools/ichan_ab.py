"""In-process A/B of the synthesis channeliser's kernels (MI355X).

Per shape (M, K), complex f32 with real f32 taps, one stream of 2^log2n samples per call:
  ring        sd.ChannelSynthesizer on the ring kernel at its automatic frames per workgroup
  ring_fN     the ring kernel at N frames per workgroup (--sweep): the sweep behind the automatic rule
  per_frame   the per-frame kernel (K transforms per frame)
  chan        the analysis sd.Channelizer at the same shape and taps
  copy        sdsp_bandwidth_copy_device over the same 16 B per sample (8 read, 8 written): the byte
              model of the ring kernel, up to its (K-1)/F warm-up reads
Untimed settle passes over every contestant come before each round; within a round the order is
shuffled; each call is timed with device events on one stream (one call per window: two medians
whose min .. max spreads overlap are reported as indistinguishable, not as a difference).  Every
synthesis contestant's output is compared bit for bit with the per-frame kernel's at the timed size.
One JSON document on stdout and in --out.

    python tools/ichan_ab.py --log2n 27 --rounds 6 --out profiles/r17/ichan_ab.json
"""
import argparse
import json
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(1024, 8), (64, 8)]  # (M, K): bench config 5's shape and a small-M one
TUNE_ICHAN_KERNEL, TUNE_ICHAN_FRAMES_PER_BLOCK = 25, 26
HBM_PEAK = 8.0e12  # B/s (datasheet)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=27, help="log2 of the samples per call")
    ap.add_argument("--rounds", type=int, default=6, help="timed rounds (shuffled), at least 3")
    ap.add_argument("--settle", type=int, default=1, help="untimed passes over every contestant before each round")
    ap.add_argument("--sweep", default="8,16,32,64,128,256,512", help="frames per workgroup of the ring_fN contestants")
    ap.add_argument("--seed", type=int, default=17)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.rounds >= 3
    sweep = [int(v) for v in args.sweep.split(",") if v]

    import torch
    import solid_dsp_amd as sd
    assert torch.cuda.is_available(), "ichan_ab needs an MI355X"
    n = 1 << args.log2n
    s = torch.cuda.current_stream()
    d_in = torch.empty(n, dtype=torch.complex64, device="cuda")
    sd.lib().sdsp_synth_f32_device(d_in.data_ptr(), 20250226, 0, 0, 2 * n, None)
    d_out = torch.empty(n, dtype=torch.complex64, device="cuda")
    d_ref = torch.empty(n, dtype=torch.complex64, device="cuda")
    torch.cuda.synchronize()
    rng = random.Random(args.seed)
    r0 = np.random.default_rng(args.seed)
    res = {"log2_samples": args.log2n, "rounds": args.rounds, "settle": args.settle, "pair": "RC32", "shapes": {}}
    for M, K in SHAPES:
        g = (r0.standard_normal(K * M) / np.sqrt(K * M)).astype(np.float32)  # white: nothing for a kernel to skip

        def synth(kernel, fpb=0):
            h = sd.ChannelSynthesizer(g, M, sample_dtype=np.complex64)
            h.set_tuning(TUNE_ICHAN_KERNEL, kernel)
            h.set_tuning(TUNE_ICHAN_FRAMES_PER_BLOCK, fpb)
            return h

        handles = {"ring": synth(2), "per_frame": synth(1)}
        for f in sweep:
            handles[f"ring_f{f}"] = synth(2, f)
        info = {k: list(h.info()) for k, h in handles.items()}
        assert info["ring"][0] == 2 and info["per_frame"][0] == 1, info
        chan = sd.Channelizer(g, M, sample_dtype=np.complex64)

        runs = {k: (lambda h=h: h.execute_block_device(d_in, n, d_out, s)) for k, h in handles.items()}
        runs["chan"] = lambda: chan.execute_block_device(d_in, n, d_out, s)
        runs["copy"] = lambda: sd.lib().sdsp_bandwidth_copy_device(d_in.data_ptr(), d_out.data_ptr(), 8 * n,
                                                                   sd._lib.stream_handle(s))
        # the same bits from every synthesis contestant (each on a fresh history, first call)
        handles["per_frame"].execute_block_device(d_in, n, d_ref, s)
        same = {}
        for k, h in handles.items():
            if k != "per_frame":
                h.execute_block_device(d_in, n, d_out, s)
                torch.cuda.synchronize()
                same[k] = bool(torch.equal(torch.view_as_real(d_out).view(torch.int32),
                                           torch.view_as_real(d_ref).view(torch.int32)))
        times = {k: [] for k in runs}
        for _ in range(args.rounds):
            for _ in range(args.settle):
                for f in runs.values():
                    f()
            torch.cuda.synchronize()
            order = list(runs)
            rng.shuffle(order)
            for k in order:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                runs[k]()
                e1.record(s)
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1))
        med = {k: float(np.median(v)) for k, v in times.items()}
        lo = {k: float(np.min(v)) for k, v in times.items()}
        hi = {k: float(np.max(v)) for k, v in times.items()}
        model = 16 * n  # bytes: every sample read once and written once

        def apart(a, b):
            return bool(hi[a] < lo[b] or hi[b] < lo[a])

        best = min((k for k in handles if k.startswith("ring")), key=lambda k: med[k])
        res["shapes"][f"M{M}_K{K}"] = {
            "samples": n, "frames": n // M, "kernel_and_frames_per_block": info,
            "bit_identical_to_per_frame": same,
            "median_ms": med, "min_ms": lo, "max_ms": hi,
            "model_bytes": model,
            "model_GBps": {k: model / (med[k] * 1e-3) / 1e9 for k in runs},
            "fraction_of_8TBps": {k: model / (med[k] * 1e-3) / HBM_PEAK for k in runs},
            "ring_lds_bytes": (K + 1) * M * 8,
            "ring_workgroups_per_cu_by_lds": (160 * 1024) // ((K + 1) * M * 8),
            "per_frame_over_ring": med["per_frame"] / med["ring"],
            "ring_over_copy": med["ring"] / med["copy"],
            "per_frame_over_copy": med["per_frame"] / med["copy"],
            "ring_over_chan": med["ring"] / med["chan"],
            "ring_vs_per_frame_distinguishable": apart("ring", "per_frame"),
            "fastest_ring": best,
            "fastest_ring_vs_automatic_distinguishable": best != "ring" and apart(best, "ring"),
        }
        del handles, chan, runs
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
