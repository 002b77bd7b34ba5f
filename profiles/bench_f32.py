"""What the exact-fp32 mode costs: the ResNet50-CAM forward at the bench shape (64 samples = 32 images x [orig, flip] at
321 x 321) in PREC_F32 and, in the same process on the same device, in PREC_F16X3 -- not the contract bench (bench.py).

    python profiles/bench_f32.py [--steps 20] [--warmup 3] [--images 32]
Conv-class milliseconds per forward from the ctx profiler (wsc_profile_begin / _end: every conv launch bracketed by events),
wall milliseconds per forward, and the conv stack's algorithmic TFLOP/s against the 155 TFLOP/s the fp32-input MFMA
(v_mfma_f32_32x32x2_f32) measures at.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "wsss-analysis_amd"))

F32_MFMA_PEAK_TFLOPS = 155.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--images", type=int, default=32)
    args = ap.parse_args()
    import numpy as np

    from wsscam import _lib, synth

    ctx = _lib.Context(0)
    B, S, C = args.images, 321, 20
    sd = synth.resnet50_cam_state_dict(C, 0)
    rng = np.random.default_rng(0)
    x_dev = ctx.to_device(rng.normal(0, 1, (B, 2, 3, S, S)).astype(np.float32))
    out = {}
    for name, prec in (("f32", _lib.PREC_F32), ("f16x3", _lib.PREC_F16X3)):
        net = _lib.Net(ctx, _lib.ARCH_RESNET50_CAM, sd, C, prec)
        h = net.cam_size_hw(S, S)[0]
        cam_dev = ctx.alloc(B * C * h * h * 4)
        for _ in range(args.warmup):
            net.forward_cam(x_dev, B, S, cam_dev)
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            net.forward_cam(x_dev, B, S, cam_dev)
        ctx.sync()
        wall = (time.perf_counter() - t0) / args.steps * 1e3
        ctx.profile_begin()
        for _ in range(args.steps):
            net.forward_cam(x_dev, B, S, cam_dev)
        prof = ctx.profile_end()
        conv = {k: v for k, v in prof.items() if k.startswith("conv_igemm_kernel")}
        conv_ms = sum(v[1] for v in conv.values()) / args.steps
        flops = sum(v[2] for v in conv.values()) / args.steps
        out[name] = {"conv_ms": round(conv_ms, 3), "other_ms": round(sum(v[1] for k, v in prof.items() if k not in conv) / args.steps, 3),
                     "wall_ms": round(wall, 3), "conv_GFLOP": round(flops / 1e9, 1), "conv_TFLOPs": round(flops / conv_ms / 1e9, 1),
                     "classes": {k: [v[0] // args.steps, round(v[1] / args.steps, 3)] for k, v in prof.items()}}
        cam_dev.free()
        net.close()
    out["f32_over_f16x3_conv"] = round(out["f32"]["conv_ms"] / out["f16x3"]["conv_ms"], 2)
    out["f32_fraction_of_mfma_peak"] = round(out["f32"]["conv_TFLOPs"] / F32_MFMA_PEAK_TFLOPS, 3)
    out["workload"] = "ResNet50-CAM forward, %d samples @%d" % (2 * B, S)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
