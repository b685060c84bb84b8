"""In-process A/B of the oversampled channeliser's kernels (MI355X).

Per shape (M, K, D), complex f32 with real f32 taps, one stream of 2^log2n input samples per call
(at D = 3M/4 the largest multiple of 3M below that), n M / D output samples:
  auto        sd.OversampledChannelizer as it comes (automatic kernel and frames per workgroup)
  per_frame   the per-frame kernel
  slide_fN    the sliding kernel at N frames per workgroup (--sweep): the sweep behind the automatic rule
  copy        sdsp_bandwidth_copy_device moving the byte model's bytes (8 per input sample read, 8 M / D
              written; the sliding kernel's model up to its (K M - D) / (F D) fill reads): half of them
              read and half written
  chan_calls  where D divides M: the M / D sd.Channelizer calls on views shifted by D samples that a
              caller needs today, without the interleave and the per-channel rotation that must follow
              them, so a lower bound of the existing path (each call one frame short, to stay inside
              the block).  At D = M this is sd.Channelizer itself
Untimed settle passes over every contestant come before each round; within a round the order is
shuffled; each call is timed with device events on one stream (one call per window: two medians
whose min .. max spreads overlap are reported as indistinguishable, not as a difference).  Every
oversampled contestant's output is compared bit for bit with the per-frame kernel's at the timed size.
One JSON document on stdout and in --out.

    python tools/oschan_ab.py --log2n 27 --rounds 6 --out profiles/r18/oschan_ab.json
"""
import argparse
import json
import math
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

K = 8
SHAPES = [(M, K, D) for M in (1024, 64) for D in (M // 2, 3 * M // 4, M)]
SHAPES += [(M, K, M // 2) for M in (128, 256, 512)]  # between the two: where the automatic choice changes kernel
TUNE_OSCHAN_KERNEL, TUNE_OSCHAN_FRAMES_PER_BLOCK = 27, 28


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=27, help="log2 of the input samples per call")
    ap.add_argument("--rounds", type=int, default=6, help="timed rounds (shuffled), at least 3")
    ap.add_argument("--settle", type=int, default=1, help="untimed passes over every contestant before each round")
    ap.add_argument("--sweep", default="8,16,32,64,128,256,512", help="frames per workgroup of the slide_fN contestants")
    ap.add_argument("--seed", type=int, default=18)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.rounds >= 3
    sweep = [int(v) for v in args.sweep.split(",") if v]

    import torch
    import solid_dsp_amd as sd
    assert torch.cuda.is_available(), "oschan_ab needs an MI355X"
    n_all = 1 << args.log2n
    s = torch.cuda.current_stream()
    d_in = torch.empty(n_all, dtype=torch.complex64, device="cuda")
    sd.lib().sdsp_synth_f32_device(d_in.data_ptr(), 20250226, 0, 0, 2 * n_all, None)
    most = 2 * n_all  # output samples at the largest M / D
    d_out = torch.empty(most, dtype=torch.complex64, device="cuda")
    d_ref = torch.empty(most, dtype=torch.complex64, device="cuda")
    torch.cuda.synchronize()
    rng = random.Random(args.seed)
    r0 = np.random.default_rng(args.seed)
    res = {"log2_samples": args.log2n, "rounds": args.rounds, "settle": args.settle, "pair": "RC32", "shapes": {}}
    for M, K_, D in SHAPES:
        n = n_all // math.lcm(M, D) * math.lcm(M, D)  # whole frames of both strides (2^log2n but for D = 3M/4)
        assert n % D == 0 and n % M == 0 and n * M // D <= most
        h = (r0.standard_normal(K_ * M) / np.sqrt(K_ * M)).astype(np.float32)  # white: nothing for a kernel to skip
        n_out = n * M // D

        def osc(kernel, fpb=0):
            c = sd.OversampledChannelizer(h, M, D, sample_dtype=np.complex64)
            c.set_tuning(TUNE_OSCHAN_KERNEL, kernel)
            c.set_tuning(TUNE_OSCHAN_FRAMES_PER_BLOCK, fpb)
            return c

        handles = {"auto": osc(0), "per_frame": osc(1)}
        for f in sweep:
            handles[f"slide_f{f}"] = osc(2, f)
        info = {k: list(c.info()) for k, c in handles.items()}
        assert info["per_frame"][0] == 1 and all(info[f"slide_f{f}"][0] == 2 for f in sweep), info

        runs = {k: (lambda c=c: c.execute_block_device(d_in, n, d_out, s)) for k, c in handles.items()}
        model = 8 * n + 8 * n_out  # bytes: every input sample read once, every output sample written once
        runs["copy"] = lambda: sd.lib().sdsp_bandwidth_copy_device(d_ref.data_ptr(), d_out.data_ptr(), model // 2,
                                                                   sd._lib.stream_handle(s))
        chans = []
        if M % D == 0:
            chans = [sd.Channelizer(h, M, sample_dtype=np.complex64) for _ in range(M // D)]
            nc = n - M if M // D > 1 else n  # a view shifted by j D samples holds one frame less

            def chan_calls():
                for j, c in enumerate(chans):
                    c.execute_block_device(d_in[j * D:j * D + nc], nc, d_out[j * nc:(j + 1) * nc], s)
            runs["chan_calls"] = chan_calls
        # the same bits from every oversampled contestant (each on a fresh history, first call)
        handles["per_frame"].execute_block_device(d_in, n, d_ref, s)
        same = {}
        for k, c in handles.items():
            if k != "per_frame":
                c.execute_block_device(d_in, n, d_out, s)
                torch.cuda.synchronize()
                same[k] = bool(torch.equal(torch.view_as_real(d_out[:n_out]).view(torch.int32),
                                           torch.view_as_real(d_ref[:n_out]).view(torch.int32)))
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

        def apart(a, b):
            return bool(hi[a] < lo[b] or hi[b] < lo[a])

        best = min((k for k in handles if k.startswith("slide")), key=lambda k: med[k])
        lds = (K_ * M + D + 3 * M) * 8
        shape = {
            "input_samples": n, "frames": n // D, "output_samples": n_out, "kernel_and_frames_per_block": info,
            "bit_identical_to_per_frame": same,
            "median_ms": med, "min_ms": lo, "max_ms": hi,
            "model_bytes": model,
            "model_GBps": {k: model / (med[k] * 1e-3) / 1e9 for k in runs},
            "fraction_of_model_at_copy_rate": {k: med["copy"] / med[k] for k in handles},
            "slide_lds_bytes": lds,
            "slide_workgroups_per_cu_by_lds": (160 * 1024) // lds,
            "per_frame_over_auto": med["per_frame"] / med["auto"],
            "auto_vs_per_frame_distinguishable": apart("auto", "per_frame"),
            "auto_slower_than_per_frame_ranges_apart": bool(lo["auto"] > hi["per_frame"]),
            "fastest_slide": best,
            "fastest_slide_vs_auto_distinguishable": apart(best, "auto"),
        }
        if chans:
            shape["chan_calls"] = M // D
            shape["chan_calls_over_auto"] = med["chan_calls"] / med["auto"]
            shape["chan_calls_vs_auto_distinguishable"] = apart("chan_calls", "auto")
        res["shapes"][f"M{M}_K{K_}_D{D}"] = shape
        del handles, chans, runs
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
