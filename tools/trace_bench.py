#!/usr/bin/env python
"""dev: what the ray queries cost (rs_trace_closest_device, rs_trace_occluded_device), and whether a scene mode's own
k_trace instantiation earns its place next to the generic one.

Rays: a scene's 800 x 500 x 16 stratum-centre camera rays (rs_probe_camera with centres = 1), device resident, tmax =
+inf, in pixel order (a pixel's 16 samples adjacent: coherent) and in a fixed seeded shuffle (what a caller's rays will
be). Scenes: `bench` (RTIOW 13.1, spheres mode), `mesh` (the C5 config's 72k-triangle mesh, flat mode), `quadric` (the
C4 config's sdl/quadric.sdl, nest mode: the generic instantiation is its own).

Variants per scene and order, alternating call by call in one process: the scene mode's own instantiation and the
generic one (RS_TRACE_GENERIC=1, read per call by the dev build of the library: run with
RS_HIP_LIB=raysnail_amd/lib/libraysnail_hip_dev.so after `make -C raysnail_amd/csrc dev`), each in the closest form
(ids + geom, no uv) and in the occlusion form; on `bench` also rs_render_features_device at 16 spp, which traces the same
first hits through the generic World::hit and makes the rays and reduces them as well. HIP events around each
asynchronous call on torch's current stream; `rounds` rounds of `reps` timed calls per variant after `warmup` calls.
Reported per variant: the median over all timed calls in ms, the range of the round medians, Mrays/s, and for the
generic variants the own instantiation's margin over them. The two instantiations' outputs are compared bit for bit
first (ids and geom where one object alone is hit; hit flag and t1 everywhere).
usage: python tools/trace_bench.py [--scenes bench,mesh,quadric] [--rounds 5] [--reps 10] [--warmup 3] [--out FILE.jsonl]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

W, H, SPP = 800, 500, 16


def timed(torch, variants, rounds, reps, warmup):
    """{name: [[ms of each timed call] per round]}, the variants alternating call by call"""
    for _ in range(warmup):
        for call in variants.values():
            call()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(rounds):
        ev = {name: [] for name in variants}
        for _ in range(reps):
            for name, call in variants.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                call()
                b.record()
                ev[name].append((a, b))
        torch.cuda.synchronize()
        for name in variants:
            times[name].append([a.elapsed_time(b) for a, b in ev[name]])
    return times


def summary(times, name):
    rmed = [statistics.median(r) for r in times[name]]
    return {"calls": sum(len(r) for r in times[name]), "ms_median": round(statistics.median(t for r in times[name] for t in r), 5),
            "ms_round_medians_min": round(min(rmed), 5), "ms_round_medians_max": round(max(rmed), 5)}


def camera_rays(ds, cam, st) -> np.ndarray:
    """(W H SPP, 8): the stratum-centre camera rays in pixel order (a pixel's samples adjacent), tmax = +inf"""
    px = np.arange(W * H, dtype=np.uint32)
    xys = np.empty((W * H, SPP, 3), np.uint32)
    xys[:, :, 0] = (px % W)[:, None]
    xys[:, :, 1] = (px // W)[:, None]
    xys[:, :, 2] = np.arange(SPP, dtype=np.uint32)[None, :]
    xys = xys.reshape(-1, 3)
    out = np.zeros((len(xys), 11))
    rc = ds.lib.rs_probe_camera(ds.handle, C.byref(cam.desc), C.byref(st), xys.ctypes.data, len(xys), 1, out.ctypes.data)
    assert rc == 0, rc
    rays = np.empty((len(xys), 8))
    rays[:, :7] = out[:, :7]
    rays[:, 7] = np.inf
    return rays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="bench,mesh,quadric")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from raysnail_amd import scenes
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    dev_lib = "_dev" in os.path.basename(os.environ.get("RS_HIP_LIB", ""))
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    builders = {"bench": lambda: scenes.rtow_13_1(W, H)[:2], "mesh": lambda: scenes.mesh_scene(W, H)[:2],
                "quadric": lambda: scenes.quadric_sdl(W, H)[:2]}
    stream = torch.cuda.current_stream().cuda_stream
    for key in filter(None, args.scenes.split(",")):
        cam, world = builders[key]()
        ds = world.device_scene()
        mode = int(ds.info().scene_mode)
        st = cam.take_photo().samples(SPP).seed(1).settings()
        host = camera_rays(ds, cam, st)
        n = len(host)
        d_pix = torch.from_numpy(host).cuda()
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(18)).cuda()
        d_shuf = d_pix[perm].contiguous()
        del host
        d_ids = torch.empty((n, 4), dtype=torch.int32, device="cuda")
        d_geom = torch.empty((n, 8), dtype=torch.float64, device="cuda")
        d_occ = torch.empty((n,), dtype=torch.uint8, device="cuda")

        def closest(rays, generic):
            os.environ.pop("RS_TRACE_GENERIC", None)
            if generic:
                os.environ["RS_TRACE_GENERIC"] = "1"
            ds.trace_closest_device(rays.data_ptr(), n, 1e-4, d_ids.data_ptr(), d_geom.data_ptr(), 0, stream)

        def occluded(rays, generic):
            os.environ.pop("RS_TRACE_GENERIC", None)
            if generic:
                os.environ["RS_TRACE_GENERIC"] = "1"
            ds.trace_occluded_device(rays.data_ptr(), n, 1e-4, d_occ.data_ptr(), stream)

        # the scene mode's own instantiation where it has one (spheres 1, flat 2) and the dev library can bypass it
        both = dev_lib and mode in (1, 2)
        if both:  # the two instantiations agree: flag and t1 everywhere, the whole row where the flag's object is the same
            closest(d_shuf, False)
            own = (d_ids.clone(), d_geom.clone())
            occluded(d_shuf, False)
            own_occ = d_occ.clone()
            closest(d_shuf, True)
            occluded(d_shuf, True)
            torch.cuda.synchronize()
            assert torch.equal(own[0][:, 0], d_ids[:, 0]) and torch.equal(own[1][:, 0].view(torch.int64), d_geom[:, 0].view(torch.int64))
            same_obj = own[0][:, 3] == d_ids[:, 3]
            assert torch.equal(own[0][same_obj], d_ids[same_obj])
            assert torch.equal(own[1][same_obj].view(torch.int64), d_geom[same_obj].view(torch.int64))
            assert torch.equal(own_occ, d_occ) and torch.equal(own_occ, d_ids[:, 0].to(torch.uint8))
            emit({"what": "agreement", "scene": key, "rays": n, "hit_share": round(float(d_occ.float().mean()), 4),
                  "rows_with_another_tied_object": int((~same_obj).sum())})
        for order, rays in (("pixel", d_pix), ("shuffled", d_shuf)):
            variants = {"closest_own": lambda rays=rays: closest(rays, False),
                        "occluded_own": lambda rays=rays: occluded(rays, False)}
            if both:
                variants["closest_generic"] = lambda rays=rays: closest(rays, True)
                variants["occluded_generic"] = lambda rays=rays: occluded(rays, True)
            if key == "bench" and order == "pixel":
                alb = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
                nrm = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
                variants["features_16spp"] = lambda: ds.render_features_device(cam.desc, st, alb.data_ptr(), nrm.data_ptr(),
                                                                               stream, stats=False)
            times = timed(torch, variants, args.rounds, args.reps, args.warmup)
            for name in variants:
                rec = {"what": "trace", "scene": key, "scene_mode": mode, "order": order, "rays": n, "variant": name}
                rec.update(summary(times, name))
                rec["Mrays_per_s"] = round(n / rec["ms_median"] / 1e3, 1)
                if name.endswith("_generic"):
                    own_ms = summary(times, name.replace("_generic", "_own"))["ms_median"]
                    rec["own_over_generic"] = round(own_ms / rec["ms_median"], 4)
                emit(rec)
        os.environ.pop("RS_TRACE_GENERIC", None)
        del d_pix, d_shuf, d_ids, d_geom, d_occ, ds, world
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
