"""Throughput of the ray-query kernel (rt_trace_rays_async) against the diagnostic build's naive
one-ray-per-thread launch (RT_QUERY_NAIVE=1), on the same GPU in the same session.
    python scripts/query_probe.py [--out DIR] [--reps 20] [--inner 10] [--scenes 1,7] [--variants SPEC]
SPEC: name:VAR=value,VAR=value;name:... -- the diagnostic build's switches each variant's scene is uploaded
with (default: persistent:RT_QUERY_NAIVE=0;naive:RT_QUERY_NAIVE=1; also RT_QUERY_STEPS, RT_QUERY_LDS).
Scenes 1 (spheres under a BVH: the kFeatBook1 instantiation, 256-thread workgroups) and 7 (every feature:
kFeatAll, the 1024-thread workgroup with the whole preorder in LDS); three batches of 810 000 rays each:
  camera    the pixel-centre rays of the scene's camera in row order (1200x675; scene 7 is square: 900x900)
  shuffled  the same rays in a random order
  random    rays from random origins inside the scene's bounds in random directions
Each repeat brackets `inner` back-to-back launches with HIP events (created on the HIP runtime the library
itself uses) and reports the time per launch; the variants alternate repeat by repeat.  Per variant
and batch: median, min and max Mrays/s over the repeats.  All variants must return identical records.
Writes query_probe.json and query_probe.md (the table of DESIGN.md §4.5) into DIR."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ray-tracing-c_amd"))
import torch  # noqa: E402  (initialised before rtc: see rtc._init_torch_runtime_first)
import rtc  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "query"))
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--inner", type=int, default=10)
ap.add_argument("--scenes", default="1,7")
ap.add_argument("--variants", default="persistent:RT_QUERY_NAIVE=0;naive:RT_QUERY_NAIVE=1")
args = ap.parse_args()
N = 810_000
VARIANTS = {v.split(":")[0]: dict(kv.split("=") for kv in v.split(":")[1].split(",") if kv) for v in args.variants.split(";")}
WIDTH = {1: 1200, 7: 900}

if rtc.device_count() < 1:
    raise SystemExit("no HIP device visible: nothing can be measured here")
os.environ.setdefault("RTC_SUBSTITUTE_EARTH", "1")
with rtc.use_diag():
    L = rtc.lib()
hip = ctypes.CDLL("libamdhip64.so")  # the runtime the library is linked to (already loaded)
for fn in ("hipEventCreate", "hipEventRecord", "hipEventSynchronize", "hipDeviceSynchronize"):
    getattr(hip, fn).restype = ctypes.c_int
hip.hipEventElapsedTime.restype = ctypes.c_int


def hip_ok(rc, what):
    if rc != 0:
        raise SystemExit(f"{what} failed with HIP error {rc}")


ev = [ctypes.c_void_p(), ctypes.c_void_p()]
for e in ev:
    hip_ok(hip.hipEventCreate(ctypes.byref(e)), "hipEventCreate")


def words(addr, count, n):
    if not count:
        return np.zeros((0, n), np.float32)
    return np.frombuffer((ctypes.c_float * (count * n)).from_address(addr), np.float32).reshape(count, n)


def batches(sc, g):
    cam = sc.s.camera
    f32 = np.float32
    p00, du, dv, org = (np.array(list(x), f32) for x in (cam.pixel00, cam.delta_u, cam.delta_v, cam.origin))
    pix = np.arange(cam.width * cam.height)[:N]
    i, j = (pix % cam.width).astype(f32), (pix // cam.width).astype(f32)
    d = (p00 + du * i[:, None]) + dv * j[:, None] - org
    camera = np.ascontiguousarray(np.concatenate([np.broadcast_to(org, d.shape), d], axis=1), f32)
    sph, quads = words(sc.s.spheres, sc.s.n_spheres, 8), words(sc.s.quads, sc.s.n_quads, 20)
    small = sph[sph[:, 3] < 100.0]  # (not the ground spheres of radius 1000)
    pts = [small[:, :3] - small[:, 3:4], small[:, :3] + small[:, 3:4]]
    if len(quads):
        q, u, v = quads[:, 0:3], quads[:, 4:7], quads[:, 8:11]
        pts += [q, q + u, q + v, q + u + v]
    pts = np.concatenate(pts)
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    rnd = np.concatenate([lo + g.random((N, 3)) * (hi - lo), g.normal(size=(N, 3))], axis=1).astype(f32)
    return {"camera": camera, "shuffled": np.ascontiguousarray(camera[g.permutation(len(camera))]), "random": rnd}


def time_launches(ds, rays, hits, prm):
    hip_ok(hip.hipEventRecord(ev[0], None), "hipEventRecord")
    for _ in range(args.inner):
        rc = L.rt_trace_rays_async(ds._h, ctypes.c_void_p(rays.data_ptr()), rays.shape[0], ctypes.byref(prm),
                                   ctypes.c_void_p(hits.data_ptr()), None)
        if rc != 0:
            raise SystemExit(f"rt_trace_rays_async: {rtc.last_error(L)}")
    hip_ok(hip.hipEventRecord(ev[1], None), "hipEventRecord")
    hip_ok(hip.hipEventSynchronize(ev[1]), "hipEventSynchronize")
    ms = ctypes.c_float()
    hip_ok(hip.hipEventElapsedTime(ctypes.byref(ms), ev[0], ev[1]), "hipEventElapsedTime")
    return ms.value / args.inner


result = {"build": L.rt_build_id().decode(), "variants": VARIANTS, "box": rtc.box_identity(0), "reps": args.reps, "inner": args.inner,
          "rays": N, "rows": []}
print(f"build={result['build']} box={result['box']}", flush=True)
prm = rtc.RtQueryParams(1e-3, float("inf"), 0, 0)
for scene_id in (int(x) for x in args.scenes.split(",")):
    with rtc.use_diag():
        sc = rtc.Scene.preset(scene_id, WIDTH.get(scene_id, 1200), 1, 1)
        variants = {}
        for v, env in VARIANTS.items():  # (the switches are read at upload)
            os.environ.update(env)
            variants[v] = rtc.DeviceScene(sc, 0)
            for k in env:
                del os.environ[k]
    for name, rays_np in batches(sc, np.random.default_rng(scene_id)).items():
        rays = torch.from_numpy(rays_np).to("cuda:0")
        hits = {v: torch.empty((len(rays_np), 12), dtype=torch.int32, device="cuda:0") for v in variants}
        torch.cuda.synchronize()
        for v, ds in variants.items():  # warm-up (the first query also makes the scene's query state)
            time_launches(ds, rays, hits[v], prm)
        hip_ok(hip.hipDeviceSynchronize(), "hipDeviceSynchronize")
        first = next(iter(hits.values()))
        same = all(bool((h == first).all()) for h in hits.values())
        ms = {v: [] for v in variants}
        for _ in range(args.reps):
            for v, ds in variants.items():
                ms[v].append(time_launches(ds, rays, hits[v], prm))
        for v in variants:
            rate = np.sort(len(rays_np) / (np.array(ms[v]) * 1e-3) / 1e6)  # Mrays/s per repeat
            row = {"scene": scene_id, "batch": name, "variant": v, "median_mrays": float(np.median(rate)),
                   "min_mrays": float(rate[0]), "max_mrays": float(rate[-1]), "median_ms": float(np.median(ms[v])),
                   "identical": same, "hit_fraction": float((hits[v][:, 9] >= 0).float().mean())}
            result["rows"].append(row)
            print(row, flush=True)
    for ds in variants.values():
        ds.close()

os.makedirs(args.out, exist_ok=True)
with open(os.path.join(args.out, "query_probe.json"), "w") as f:
    json.dump(result, f, indent=1)
with open(os.path.join(args.out, "query_probe.md"), "w") as f:
    f.write(f"build `{result['build']}`, {N} rays per batch, {args.reps} repeats of {args.inner} launches, "
            f"box {result['box'].get('host', '?')}\n\n")
    f.write("| scene | batch | variant | Mrays/s median | min | max | ms per launch | identical |\n|---|---|---|---|---|---|---|---|\n")
    for r in result["rows"]:
        f.write(f"| {r['scene']} | {r['batch']} | {r['variant']} | {r['median_mrays']:.0f} | {r['min_mrays']:.0f} | "
                f"{r['max_mrays']:.0f} | {r['median_ms']:.3f} | {r['identical']} |\n")
print("wrote", os.path.join(args.out, "query_probe.md"))
