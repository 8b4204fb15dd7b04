"""Timing helper for the AirSim driver's contract (Examples/Stereo/stereo_airsim.cc:386-411): k_resize on the input images (8UC3, image
size -> 512x512) and on the cost maps (8UC1, 512x512 -> image size) at batch 64 for 1242x375 and 1920x1200, then the resized forward
(ivf_fcn_forward_device_resized, in = out = 512x512) beside the plain one (ivf_fcn_forward_device, in = out = 1242x375, what bench.py
runs).  HIP events through torch on the launch stream; run it under `rocprofv3 --kernel-trace --stats -- python tools/time_resize.py`
for per-kernel numbers."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import iv_slam_amd as iv
from iv_slam_amd import fcn_weights

N, REPS = 64, 20
HBM_PEAK_GBS = 8000.0           # MI355X HBM3E peak (MI355X_MICROARCH.md)


def timed(fn, reps=REPS):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps          # us per call


def main():
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev); g.manual_seed(1)
    for w, h in ((1242, 375), (1920, 1200)):
        src = torch.randint(0, 256, (N, h, w, 3), dtype=torch.uint8, device=dev, generator=g)
        small = torch.empty((N, 512, 512, 3), dtype=torch.uint8, device=dev)
        rin = iv.Resize((w, h), (512, 512), 3)
        us = timed(lambda: rin.apply_device(src, small))
        alg = N * (w * h * 3 + 512 * 512 * 3)
        print("input resize 8UC3 %dx%d -> 512x512, batch %d: %.1f us per launch, %.2f us per image, %.0f GB/s (%.2f of HBM peak)"
              % (w, h, N, us, us / N, alg / us / 1e3, alg / us / 1e3 / HBM_PEAK_GBS))
        cmap = torch.randint(0, 256, (N, 512, 512), dtype=torch.uint8, device=dev, generator=g)
        big = torch.empty((N, h, w), dtype=torch.uint8, device=dev)
        rout = iv.Resize((512, 512), (w, h), 1)
        us2 = timed(lambda: rout.apply_device(cmap, big))
        alg = N * (512 * 512 + w * h)
        print("map resize 8UC1 512x512 -> %dx%d, batch %d: %.1f us per launch, %.2f us per image, %.0f GB/s (%.2f of HBM peak)"
              % (w, h, N, us2, us2 / N, alg / us2 / 1e3, alg / us2 / 1e3 / HBM_PEAK_GBS))
        print("both resizes at %dx%d: %.2f us per image" % (w, h, (us + us2) / N))
    # the forward passes at 1242x375, batch 64
    w, h = 1242, 375
    blob = fcn_weights.pack_blob(fcn_weights.make_seeded_weights(5))
    bgr = torch.randint(0, 256, (N, h, w, 3), dtype=torch.uint8, device=dev, generator=g)
    cost = torch.empty((N, h, w), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    plain = iv.IntrospectionFCN(blob, (h, w), (h, w), max_batch=N)
    us_p = timed(lambda: plain.forward_device(bgr, cost_u8=cost, stream_ptr=stream), reps=5)
    plain.status(stream)
    del plain
    rs = iv.IntrospectionFCN(blob, (512, 512), (512, 512), max_batch=N)
    us_r = timed(lambda: rs.forward_device_resized(bgr, cost, (w, h), stream), reps=5)
    rs.status(stream)
    print("forward %dx%d batch %d: plain (in = out = image size) %.1f us per image; resized (stereo_airsim.cc contract, in = out = 512x512) "
          "%.1f us per image" % (w, h, N, us_p / N, us_r / N))


if __name__ == "__main__":
    main()
