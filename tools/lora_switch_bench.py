"""What one adapter switch costs at the 14B block shapes: ops.lora_merge (csrc/ce_lora.hip) over the twelve Linears of a block -
self- and cross-attention q / k / v / out and the two image-context projections at 5120 x 5120, FFN up 13824 x 5120, FFN down
5120 x 13824 - with one adapter of rank 32 and of rank 128 on every one of them, against the arithmetic of fuse_lora on the same
shapes (`w.float() + s * (b.float() @ a.float())` rounded to bf16: what the parent commit runs once per adapter on a freshly loaded
model, with no way back).  Several blocks' worth of distinct buffers are walked so that nothing is served from the caches; the
whole-model figure is the per-block time x 40.  Prints the time, the achieved GB/s (4 bytes per weight element: read base, write
weight) and the memory the base store adds.

    timeout 300 python tools/lora_switch_bench.py [--blocks 4] [--reps 5]

(--time-limit: the script also ends itself after that many seconds.)"""
import argparse
import os
import signal
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from chronoedit_amd import ops  # noqa: E402

D, F, LAYERS = 5120, 13824, 40
BLOCK_SHAPES = [(D, D)] * 10 + [(F, D), (D, F)]  # (out_features, in_features)


def _time(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st.record()
        fn()
        en.record()
        en.synchronize()
        ts.append(st.elapsed_time(en) * 1e-3)
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=4, help="blocks' worth of distinct weights walked per timed pass")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--time-limit", type=int, default=280)
    args = ap.parse_args()
    signal.alarm(args.time_limit)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: (torch.randn(s, generator=g, device=dev) * 0.05).to(torch.bfloat16)
    base = [[rnd(n, k) for n, k in BLOCK_SHAPES] for _ in range(args.blocks)]
    live = [[torch.empty_like(w) for w in blk] for blk in base]
    elems = sum(n * k for n, k in BLOCK_SHAPES)
    print(f"block: {len(BLOCK_SHAPES)} Linears, {elems / 1e6:.1f} M weights; base store of an adapter on all of them: "
          f"{elems * 2 * LAYERS / 2**30:.1f} GiB for {LAYERS} blocks")

    def copy_pass():
        for bb, lb in zip(base, live):
            for w0, w in zip(bb, lb):
                w.copy_(w0)

    t = _time(copy_pass, args.reps) / args.blocks
    print(f"torch copy (the streaming rate to compare with): {t * 1e3:8.3f} ms / block  {4 * elems / t / 1e9:7.0f} GB/s  -> {t * LAYERS * 1e3:7.1f} ms / model")

    def merge_pass(ad):
        for bb, lb, ab in zip(base, live, ad):
            for w0, w, adapters in zip(bb, lb, ab):
                ops.lora_merge(w0, adapters, out=w)

    zero = [[[] for _ in blk] for blk in base]
    t = _time(lambda: merge_pass(zero), args.reps) / args.blocks
    print(f"lora_merge, no adapter (disable_lora):          {t * 1e3:8.3f} ms / block  {4 * elems / t / 1e9:7.0f} GB/s  -> {t * LAYERS * 1e3:7.1f} ms / model")
    for ranks in ([32], [128], [128, 32]):
        ad = [[[(rnd(r, k), rnd(n, r), 0.5) for r in ranks] for n, k in BLOCK_SHAPES] for _ in range(args.blocks)]
        t = _time(lambda: merge_pass(ad), args.reps) / args.blocks
        flops = 2.0 * elems * sum(ranks)
        print(f"lora_merge, ranks {str(ranks):10s}:                 {t * 1e3:8.3f} ms / block  {4 * elems / t / 1e9:7.0f} GB/s  -> {t * LAYERS * 1e3:7.1f} ms / model"
              f"   ({flops / t / 1e12:.0f} TFLOP/s of rank products)")

        def fuse_pass():  # the arithmetic of LoraMixin.fuse_lora, one adapter after the other, in place
            for lb, ab in zip(live, ad):
                for w, adapters in zip(lb, ab):
                    for a, b, s in adapters:
                        w.copy_((w.float() + s * (b.float() @ a.float())).to(w.dtype))

        t = _time(fuse_pass, max(2, args.reps // 2)) / args.blocks
        print(f"fuse_lora arithmetic, ranks {str(ranks):10s}:       {t * 1e3:8.3f} ms / block  {'':7s}       -> {t * LAYERS * 1e3:7.1f} ms / model")
        del ad


if __name__ == "__main__":
    main()
