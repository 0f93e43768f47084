# dev: a matrix of small frames over the host render path's schemes and entry points; per frame the statistics that
# witness the launch plan (launches, kernel_launches count what the host enqueued) and a SHA-256 of the frame. Two
# libraries that enqueue the same work print identical text: RS_HIP_LIB=<library> python tools/render_matrix.py
import hashlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
torch.cuda.set_device(0)
from raysnail_amd import _abi as A
from raysnail_amd import api, scenes

W, H = 160, 100
S = torch.cuda.current_stream().cuda_stream


def line(name, frame, st):
    sha = hashlib.sha256(np.ascontiguousarray(frame).tobytes()).hexdigest()[:16]
    print(f"{name:34s} samples {st.samples} segments {st.segments} launches {st.launches} kernel_launches "
          f"{st.kernel_launches} kernel_bytes {st.kernel_bytes} kernel_id {st.kernel_id} sha {sha}", flush=True)


def host(name, ds, cam, st, mask=None, reps=1):
    for r in range(reps):
        out, stats = ds.render(cam.desc, st, mask)
        line(f"{name} #{r}", out, stats)


def passes(name, ds, cam, photo):
    outs = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(3)]
    stats = ds.render_device_passes(cam.desc, photo.pass_index(2).settings(), [o.data_ptr() for o in outs], S)
    torch.cuda.synchronize()
    line(name, np.stack([o.cpu().numpy() for o in outs]), stats)


mask = (np.indices((H, W)).sum(0) % 5 != 0).astype(np.uint8)
cam, world, _, _ = scenes.rtow_13_1(W, H)
for lanes in (1, 2):
    for tag, depth, ws in (("d8", 8, None), ("d50", 50, None), ("ws", 8, (96 * 60, 96 * 60 * 16))):
        ds = api.DeviceScene(world)
        ds.set_lanes(lanes)
        if ws:
            ds.set_workspace(*ws)
        host(f"rtow {tag} lanes {lanes}", ds, cam, cam.take_photo().samples(16).depth(depth).seed(3).settings(), reps=3)
ds = api.DeviceScene(world)
photo = cam.take_photo().samples(16).depth(8).seed(3)
host("rtow mega", ds, cam, cam.take_photo().samples(16).depth(8).seed(3).mode(A.RS_MODE_MEGAKERNEL).settings())
host("rtow samples 1 depth 0", ds, cam, cam.take_photo().samples(1).depth(0).seed(3).settings())
host("rtow samples 0", ds, cam, cam.take_photo().samples(0).depth(8).seed(3).settings())
host("rtow rows 0::8", ds, cam, cam.take_photo().samples(16).depth(8).seed(3).rows(0, 0, 8).settings())
seen = []
out, stats = ds.render_rows(cam.desc, photo.settings(), lambda y, o: seen.append(y), mask, bands=7, stats=True)
line(f"rtow render_rows bands 7 ({len(seen)} calls)", out, stats)
passes("rtow passes 3 (stream)", ds, cam, photo)
t = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
d_mask = torch.from_numpy(mask).cuda()
ds2 = api.DeviceScene(world, devices=[0, 0])
host("rtow devices [0, 0] mask", ds2, cam, photo.settings(), mask)
stats = ds2.render_device(cam.desc, photo.settings(), t.data_ptr(), S, d_mask.data_ptr())
line("rtow devices [0, 0] device mask", t.cpu().numpy(), stats)
for name, (c, w) in (("example", scenes.example_sdl(W, H)), ("quadric", scenes.quadric_sdl(W, H)),
                     ("cornell_smoke", scenes.cornell_smoke(100, 100))):
    host(name, api.DeviceScene(w), c, c.take_photo().samples(16).depth(8).seed(3).settings(), reps=2)
ds = api.DeviceScene(w)  # the rich scene again in four batches of chunks on two lanes
ds.set_workspace(100 * 100 * 4, 0)
host("cornell_smoke 4 batches", ds, c, c.take_photo().samples(16).depth(8).seed(3).settings())
cam, world = scenes.mesh_scene(W, H, 40, 80)
st = cam.take_photo().samples(16).depth(8).seed(3).settings()
for lanes in (1, 2):
    ds = api.DeviceScene(world)
    ds.set_lanes(lanes)
    host(f"mesh lanes {lanes}", ds, cam, st, reps=2)
    host(f"mesh lanes {lanes} mask", ds, cam, st, mask)
host("mesh mega", ds, cam, cam.take_photo().samples(16).depth(8).seed(3).mode(A.RS_MODE_MEGAKERNEL).settings())
passes("mesh passes 3 (falls back)", ds, cam, cam.take_photo().samples(16).depth(8).seed(3))
