"""Times of the tracking kernels at 480 x 640 (a measurement aid, no threshold):

  raycast      bf_tsdf_raycast of one view of two volumes at 2 cm voxels: "wall", mesh_probe.py's smooth wall
               fused from eight frames, seen from its first camera, and "room", a 4 x 3.5 x 2.6 m box room fused
               from four frames looking into a corner, seen from the last of them; with the counters
  live maps    bf_depth_vertex_normal of one frame
  icp_reduce   one bf_icp_reduce (both kernels) of a room frame against the room's raycast, at strides 4 / 2 / 1
  grey         bf_grey_u8 of one colour frame
  photo_reduce one bf_photo_reduce (both kernels) of that room frame against the frame before it, textured, at
               strides 4 / 2 / 1
  track        IcpTracker.track of the next room frame from the pose before it: wall-clock of the whole call, the
               raycast, the twelve reductions, their read-backs and the host's 6 x 6 solves included
  track_rgb    the same call with the frame's image: bf_grey_u8 and twelve bf_photo_reduce more, one read-back each
  fern_encode  bf_fern_encode (cell 16, 512 ferns) of one room frame with its image, and of a batch of eight
  fern_search  bf_fern_search (both kernels, k = 4) of one code against 256 and against 4096 random keyframes
  observe      Relocaliser.observe of a room frame: encode, search with k = 1 and the conditional append
  relocalise   Relocaliser.relocalise of the next room frame with the four fused frames as keyframes: wall-clock of
               the query, its read-back and the tracker's call from the nearest keyframe's pose

Device times are the median of REPS runs between device events after a warm-up, with their min and max; the
wall-clock is the median of REPS calls, each followed by a synchronisation.  --scale shrinks the image for a
rehearsal.  One JSON line at the end."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from boxfusion_amd import _lib  # noqa: E402
from boxfusion_amd.scene_mesh import TsdfVolume  # noqa: E402
from boxfusion_amd.synthetic import SCANNET_K, Scene  # noqa: E402
from boxfusion_amd.tracking import IcpTracker, Relocaliser, world_to_camera  # noqa: E402

REPS = 9
LO, HI = np.array([-2.0, -1.7, -1.3]), np.array([2.0, 1.8, 1.3])


def device_ms(fn):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return dict(ms=round(float(np.median(out)), 4), min=round(float(min(out)), 4), max=round(float(max(out)), 4))


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    fwd = (target - eye) / np.linalg.norm(target - eye)
    right = np.cross(fwd, up)
    right /= np.linalg.norm(right)
    P = np.eye(4)
    P[:3, 0], P[:3, 1], P[:3, 2], P[:3, 3] = right, np.cross(fwd, right), fwd, eye
    return P.astype(np.float32)


def room_depth(pose, K, H, W):
    """the inside of the box LO .. HI from a camera in it: the nearest exit through the six slabs"""
    P = pose.astype(np.float64)
    v, u = np.mgrid[:H, :W].astype(np.float64)
    a, b = (u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1]
    best = np.full((H, W), np.inf)
    with np.errstate(all="ignore"):
        for i in range(3):
            d = P[i, 0] * a + P[i, 1] * b + P[i, 2]
            t = np.where(d > 0, (HI[i] - P[i, 3]) / d, np.where(d < 0, (LO[i] - P[i, 3]) / d, np.inf))
            best = np.minimum(best, np.where(t > 0, t, np.inf))
    return best.astype(np.float32)


def room_image(pose, K, depth):
    """u8 [H,W,3]: a smooth texture of the world point each pixel sees"""
    P = pose.astype(np.float64)
    H, W = depth.shape
    v, u = np.mgrid[:H, :W].astype(np.float64)
    d = depth.astype(np.float64)
    a, b = (u - K[0, 2]) / K[0, 0] * d, (v - K[1, 2]) / K[1, 1] * d
    x, y, z = [P[i, 0] * a + P[i, 1] * b + P[i, 2] * d + P[i, 3] for i in range(3)]
    t = 0.5 + 0.16 * np.sin(5 * (x + z) + 1) + 0.14 * np.sin(6 * (y - z) - 0.5) + 0.10 * np.sin(3.5 * (x + y) + 2)
    return np.repeat(np.rint(255.0 * t).astype(np.uint8)[..., None], 3, -1)


def wall_depth(i, H, W):
    v, u = np.mgrid[:H, :W].astype(np.float32)
    u, v = u * (640.0 / W), v * (480.0 / H)
    return (2.2 + 0.7 * np.sin(u / 210.0 + 0.3 * i) * np.cos(v / 170.0) + 0.001 * (u - 320)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the image by this factor (rehearsal)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("track_bench: needs a HIP device")
    _lib.lib()
    dev = torch.device("cuda")
    H, W = max(int(480 * args.scale), 16), max(int(640 * args.scale), 16)
    K = np.asarray(SCANNET_K, np.float32).reshape(3, 3).copy()
    K[0] *= W / 640.0
    K[1] *= H / 480.0
    intr = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    out = dict(device=torch.cuda.get_device_name(0), hw=[H, W], reps=REPS)

    scene = Scene(seed=0)
    wall = TsdfVolume(voxel=0.02, trunc_voxels=4, capacity=1 << 16, device=dev)
    wall_poses = np.stack([scene.pose(i) for i in range(8)]).astype(np.float32)
    wall.integrate(torch.from_numpy(np.stack([wall_depth(i, H, W) for i in range(8)])).to(dev), K, wall_poses)

    room = TsdfVolume(voxel=0.02, trunc_voxels=4, capacity=1 << 16, device=dev)
    room_poses = [look_at([0.5 - 0.03 * i, 0.6 - 0.02 * i, 0.2 + 0.01 * i], [-2.0 + 0.05 * i, -1.7 + 0.03 * i, -1.3 + 0.03 * i])
                  for i in range(5)]
    room_depths = [torch.from_numpy(room_depth(p, K, H, W)).to(dev) for p in room_poses]
    room.integrate(torch.stack(room_depths[:4]), K, np.stack(room_poses[:4]))
    out["blocks"] = dict(wall=wall.stats()["blocks"], room=room.stats()["blocks"])

    for name, vol, pose in (("wall", wall, wall_poses[0]), ("room", room, room_poses[3])):
        row = device_ms(lambda: vol.raycast(pose, K, H, W))
        row.update(zip(_lib.TSDF_RAYCAST_STATS, vol.raycast(pose, K, H, W)[4].cpu().tolist()))
        out[f"raycast_{name}"] = row
        print(f"raycast {name}", row, flush=True)

    out["live_maps"] = device_ms(lambda: _lib.depth_vertex_normal(room_depths[4], intr, room.max_depth, 0.08))
    print("live maps", out["live_maps"], flush=True)
    lv, ln = _lib.depth_vertex_normal(room_depths[4], intr, room.max_depth, 0.08)
    _, mv, mn, _, _ = room.raycast(room_poses[3], K, H, W)
    T, M = room_poses[3].astype(np.float64)[:3], world_to_camera(room_poses[3])
    for stride in (4, 2, 1):
        row = device_ms(lambda: _lib.icp_reduce(lv, ln, stride, T, mv[0], mn[0], M, intr, 0.32, 0.8))
        row.update(blocks=_lib.icp_blocks(H, W, stride),
                   inliers=int(_lib.icp_reduce(lv, ln, stride, T, mv[0], mn[0], M, intr, 0.32, 0.8)[28].item()))
        out[f"icp_reduce_stride{stride}"] = row
        print(f"icp_reduce stride {stride}", row, flush=True)

    rgbs = [torch.from_numpy(room_image(room_poses[i], K, room_depths[i].cpu().numpy())).to(dev) for i in (3, 4)]
    out["grey"] = device_ms(lambda: _lib.grey_u8(rgbs[1]))
    print("grey", out["grey"], flush=True)
    ri, li, Mr = _lib.grey_u8(rgbs[0]), _lib.grey_u8(rgbs[1]), world_to_camera(room_poses[3])
    for stride in (4, 2, 1):
        row = device_ms(lambda: _lib.photo_reduce(lv, li, stride, T, ri, room_depths[3], Mr, intr, 0.32, 0.3))
        row.update(blocks=_lib.icp_blocks(H, W, stride),
                   inliers=int(_lib.photo_reduce(lv, li, stride, T, ri, room_depths[3], Mr, intr, 0.32, 0.3)[28].item()))
        out[f"photo_reduce_stride{stride}"] = row
        print(f"photo_reduce stride {stride}", row, flush=True)

    tracker = IcpTracker(room, K, H, W)
    for name, rgb in (("track", None), ("track_rgb", rgbs[1])):
        walls = []
        for _ in range(REPS + 1):                               # the first call is the warm-up
            tracker.set_reference(rgbs[0], room_depths[3], room_poses[3])     # a frame placed with its image replaces it
            torch.cuda.synchronize()
            t = time.perf_counter()
            pose, info = tracker.track(room_depths[4], room_poses[3], rgb)
            torch.cuda.synchronize()
            walls.append((time.perf_counter() - t) * 1e3)
        walls = walls[1:]
        err = float(np.linalg.norm(pose[:3, 3] - room_poses[4][:3, 3])) if not info["lost"] else None
        out[name] = dict(wall_ms=round(float(np.median(walls)), 3), min=round(min(walls), 3), max=round(max(walls), 3),
                         iterations=info["iterations"], lost=info["lost"], cond=round(info["cond"], 2),
                         inlier_share=round(info["inliers"] / max(info["sampled"], 1), 3), translation_error_m=err)
        if rgb is not None:
            out[name].update(photo_inlier_share=round(info["photo_inliers"] / max(info["sampled"], 1), 3),
                             photo_rms=round(info["photo_rms"], 5))
        print(name, out[name], flush=True)

    cell = 16 if min(H, W) >= 64 else 4
    rl = Relocaliser(H, W, dev, ferns=512, cell=cell, max_depth=room.max_depth)
    all_rgbs = [torch.from_numpy(room_image(room_poses[i], K, room_depths[i].cpu().numpy())).to(dev) for i in range(5)]
    one_d, one_c = room_depths[4][None].contiguous(), all_rgbs[4][None].contiguous()
    eight_d, eight_c = one_d.repeat(8, 1, 1), one_c.repeat(8, 1, 1, 1)
    for name, d, c in (("fern_encode_1", one_d, one_c), ("fern_encode_8", eight_d, eight_c)):
        out[name] = device_ms(lambda: _lib.fern_encode(d, c, cell, room.max_depth, rl._ferns))
        print(name, out[name], flush=True)
    rng = np.random.default_rng(0)
    table = torch.from_numpy(rng.integers(0, 1 << 32, (4096, 64), dtype=np.uint64).astype(np.uint32).view(np.int32)).to(dev)
    code = _lib.fern_encode(one_d, one_c, cell, room.max_depth, rl._ferns)
    for n in (256, 4096):
        held = torch.tensor([n], dtype=torch.int32, device=dev)
        out[f"fern_search_{n}"] = device_ms(lambda: _lib.fern_search(table, held, n, code, 4))
        print(f"fern_search {n}", out[f"fern_search_{n}"], flush=True)
    for i in range(4):
        rl.observe(room_depths[i], room_poses[i], all_rgbs[i], i)
    out["observe"] = device_ms(lambda: rl.observe(room_depths[4], room_poses[4], all_rgbs[4], 4))
    out["observe"].update(rl.counters())
    print("observe", out["observe"], flush=True)
    walls = []
    for _ in range(REPS + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        pose, info = rl.relocalise(tracker, room_depths[4], all_rgbs[4])
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t) * 1e3)
    walls = walls[1:]
    err = float(np.linalg.norm(pose[:3, 3] - room_poses[4][:3, 3])) if not info["lost"] else None
    out["relocalise"] = dict(wall_ms=round(float(np.median(walls)), 3), min=round(min(walls), 3), max=round(max(walls), 3),
                             lost=info["lost"], candidates_tried=info["candidates_tried"], keyframe=info.get("keyframe"),
                             fern_distance=info.get("fern_distance"), translation_error_m=err)
    print("relocalise", out["relocalise"], flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
