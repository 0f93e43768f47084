# dev: the first-hit feature pass against the beauty frame on the benchmark scene (RTIOW 13.1, seed 7, 800x500,
# depth 8), in one process: rs_render_features_device at 64 and at 16 spp and rs_render_device at 64 spp, the three
# alternating, each timed by the host clock around asynchronous calls that end in a stream synchronise (per frame,
# median and min over the rounds), plus the feature kernel's own device time from the call's stats.
# usage: python tools/time_features.py [rounds] [frames per round] [WxH]    (one JSON line per measurement)
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

torch.cuda.set_device(0)
from raysnail_amd import scenes  # noqa: E402

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
frames = int(sys.argv[2]) if len(sys.argv) > 2 else 20
W, H = map(int, (sys.argv[3] if len(sys.argv) > 3 else "800x500").split("x"))
cam, world, _, _ = scenes.rtow_13_1(W, H)
ds = world.device_scene()
stream = torch.cuda.current_stream().cuda_stream
a = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
n = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")


def settings(spp):
    return cam.take_photo().samples(spp).depth(8).seed(1).settings()


def features(spp):
    st = settings(spp)
    return lambda stats=False: ds.render_features_device(cam.desc, st, a.data_ptr(), n.data_ptr(), stream, stats=stats)


def beauty(spp):
    st = settings(spp)
    return lambda stats=False: ds.render_device(cam.desc, st, out.data_ptr(), stream, stats=stats)


cases = {"features_64spp": features(64), "features_16spp": features(16), "beauty_64spp": beauty(64)}
times = {k: [] for k in cases}
for k, f in cases.items():  # warm up every shape
    for _ in range(3):
        f()
torch.cuda.synchronize()
for _ in range(rounds):
    for k, f in cases.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(frames):
            f()
        torch.cuda.synchronize()
        times[k].append((time.perf_counter() - t0) / frames * 1e3)
for k, f in cases.items():
    st = f(True)
    print(json.dumps({"case": k, "size": f"{W}x{H}", "ms_per_frame_median": round(statistics.median(times[k]), 4),
                      "ms_per_frame_min": round(min(times[k]), 4), "ms_per_frame_max": round(max(times[k]), 4),
                      "rounds": rounds, "frames_per_round": frames, "samples": int(st.samples),
                      "segments": int(st.segments), "kernel_ms_timed_call": round(st.kernel_ms, 4),
                      "kernel_launches": int(st.kernel_launches),
                      "Msamples_s": round(st.samples / statistics.median(times[k]) / 1e3, 1)}), flush=True)
