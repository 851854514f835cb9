"""Batched closest-hit ray queries (include/rt_hip.h: rt_trace_rays_async / rt_trace_rays; rtc:
DeviceScene.trace_rays, trace_rays_host) against the oracle's hit methods.

The checker is tests/native/ray_query_ref.c (bin/libray_query_ref.so): the oracle's recursive `hit` over
the world, ray k's rng seeded (rng_state, rng_seq + k).  Every comparison is bit for bit.  A hit in a
ConstantMedium compares t, p, material and the flags (the reference leaves the rest stale; the API
defines it as 0).  The oracle's record has no primitive id, so `prim` is checked through its material
and, in scenes without transforms, through query_ref_prim: that primitive alone gives the same t.

Rays (fixed numpy seed, 4099 per batch -- no multiple of 64 or 256): the scene camera's pixel-centre
rays, rays from random points inside the scene's bounds in random directions, directions with one and
with two components exactly 0, directions scaled by 1e-6 and 1e6.  The API's tmax is one value per call,
so the finite tmax values are drawn from the unbounded hits' t of a random tenth of the batch (exact
elements, so a hit sits exactly on the bound: exclusive for a sphere, inclusive for a quad) and each is
applied to the whole batch: some hits are cut off, others replaced by farther ones.

Without a GPU: the kernel's per-lane code and an emulation of its wave's refill rounds on the host under
AddressSanitizer (tests/native/query_host_check.cpp).  With one: the library's one-ray-per-thread launch
and the diagnostic build's persistent lane-refilling kernel (RT_QUERY_NAIVE=0), which must agree.
"""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import rtc
from conftest import ROOT, golden_image

N = 4099
SCENES = (1, 2, 5, 6, 7)
WIDTH = 16
SEED = 20240607
REF_LIB = os.path.join(ROOT, "tests", "native", "bin", "libray_query_ref.so")
HOST = os.path.join(ROOT, "tests", "native", "bin", "query_host_check")
INF = float("inf")


# ------------------------------------------------------------------------------------ the checker
@pytest.fixture(scope="module", autouse=True)
def query_helpers_built(built):
    """The checkers of this module (tests/native/query.mk), built in-tree if missing, as conftest builds the others."""
    if not (os.path.exists(REF_LIB) and os.path.exists(HOST)):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "native"), "-f", "query.mk", "-j8"], check=True)
    yield


@functools.lru_cache(maxsize=None)
def _ref_lib():
    L = ctypes.CDLL(REF_LIB)
    L.query_ref.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(rtc.RtQueryParams),
                            ctypes.c_void_p]
    L.query_ref.restype = ctypes.c_int
    L.query_ref_prim.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_float, ctypes.c_float,
                                 ctypes.POINTER(ctypes.c_float)]
    L.query_ref_prim.restype = ctypes.c_int
    return L


def query_ref(sc, rays, tmin, tmax, rng=(0, 0)):
    rays = np.ascontiguousarray(rays, np.float32)
    hits = np.empty((rays.shape[0], 12), np.int32)
    prm = rtc.RtQueryParams(tmin, tmax, rng[0], rng[1])
    assert _ref_lib().query_ref(ctypes.cast(sc.ptr, ctypes.c_void_p), rays.ctypes.data, rays.shape[0],
                                ctypes.byref(prm), hits.ctypes.data) == 0
    return hits


def _words(addr, count, words):
    """A flat-scene array of `count` records of `words` 32-bit words as an int32 array."""
    if not count:
        return np.zeros((0, words), np.int32)
    buf = (ctypes.c_int32 * (count * words)).from_address(addr)
    return np.frombuffer(buf, np.int32).reshape(count, words)


# ------------------------------------------------------------------------------------ scenes and rays
@functools.lru_cache(maxsize=None)
def scene(scene_id, width=WIDTH):
    return rtc.Scene.preset(scene_id, width, 1, 1)


def scene_bounds(sc):
    s = sc.s
    sph = _words(s.spheres, s.n_spheres, 8).view(np.float32)
    quads = _words(s.quads, s.n_quads, 20).view(np.float32)
    pts = []
    small = sph[sph[:, 3] < 100.0]  # (not the ground spheres of radius 1000)
    if len(small):
        pts += [small[:, :3] - small[:, 3:4], small[:, :3] + small[:, 3:4]]
    if len(quads):
        q, u, v = quads[:, 0:3], quads[:, 4:7], quads[:, 8:11]
        pts += [q, q + u, q + v, q + u + v]
    pts = np.concatenate(pts)
    return pts.min(axis=0) - 1.0, pts.max(axis=0) + 1.0


@functools.lru_cache(maxsize=None)
def make_rays(scene_id, seed=SEED, width=WIDTH):
    sc = scene(scene_id, width)
    g = np.random.default_rng(seed + scene_id)
    cam = sc.s.camera
    W, H = cam.width, cam.height
    f32 = np.float32
    p00, du, dv, org = (np.array(list(x), f32) for x in (cam.pixel00, cam.delta_u, cam.delta_v, cam.origin))
    lo, hi = scene_bounds(sc)

    def origins(n):
        return (lo + g.random((n, 3)) * (hi - lo)).astype(f32)

    def directions(n):
        d = g.normal(size=(n, 3)).astype(f32)
        d[np.abs(d) < 1e-3] = 0.5  # (a component is zero only where a group below sets it)
        return d

    parts = []
    n_cam = min(W * H, 1200)
    pix = g.choice(W * H, n_cam, replace=False)
    i, j = (pix % W).astype(f32), (pix // W).astype(f32)
    d = (p00 + du * i[:, None]) + dv * j[:, None] - org
    parts.append(np.concatenate([np.broadcast_to(org, d.shape), d], axis=1))
    for n, kind in ((400, "zero1"), (300, "zero2"), (400, "tiny"), (399, "huge")):
        o, d = origins(n), directions(n)
        if kind == "zero1":
            d[np.arange(n), g.integers(0, 3, n)] = 0.0
        elif kind == "zero2":
            keep = g.integers(0, 3, n)
            for a in range(3):
                d[keep != a, a] = 0.0
        elif kind == "tiny":
            d *= f32(1e-6)
        else:
            d *= f32(1e6)
        parts.append(np.concatenate([o, d], axis=1))
    n_rand = N - sum(len(p) for p in parts)
    parts.append(np.concatenate([origins(n_rand), directions(n_rand)], axis=1))
    rays = np.ascontiguousarray(np.concatenate(parts)[g.permutation(N)], f32)
    assert rays.shape == (N, 6) and not (rays[:, 3:] == 0).all(axis=1).any()
    rays.setflags(write=False)
    return rays


@functools.lru_cache(maxsize=None)
def tmax_values(scene_id):
    """+inf, then three finite bounds: exact t values of unbounded hits among a random tenth of the batch."""
    ref = query_ref(scene(scene_id), make_rays(scene_id), 1e-3, INF)
    g = np.random.default_rng(SEED + 100 + scene_id)
    t = ref[g.choice(N, N // 10, replace=False), 0].view(np.float32)
    t = np.sort(t[np.isfinite(t)])
    assert len(t) >= 8, "the tenth holds too few hits to draw bounds from"
    return (INF,) + tuple(float(t[int(q * (len(t) - 1))]) for q in (0.25, 0.5, 0.75))


@functools.lru_cache(maxsize=None)
def reference(scene_id, tmax=INF, rng=(0, 0)):
    ref = query_ref(scene(scene_id), make_rays(scene_id), 1e-3, tmax, rng)
    ref.setflags(write=False)
    return ref


# ------------------------------------------------------------------------------------ comparison
def check_hits(sc, rays, got, ref, what, tmin=1e-3, tmax=INF, prim_t=False):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape == (len(rays), 12), what
    medium = (ref[:, 11] & rtc.HIT_IN_MEDIUM) != 0
    cols = np.ones(12, bool)
    cols[10] = False  # prim: below
    bad = (got[:, cols] != ref[:, cols]).any(axis=1) & ~medium
    mcols = [0, 1, 2, 3, 9, 11]
    bad |= ((got[:, mcols] != ref[:, mcols]).any(axis=1) | (got[:, 4:9] != 0).any(axis=1)) & medium
    assert not bad.any(), (f"{what}: {bad.sum()} of {len(rays)} records differ; first at {np.argmax(bad)}: "
                           f"ray {rays[np.argmax(bad)]}\n got {got[np.argmax(bad)]}\n ref {ref[np.argmax(bad)]}")
    # prim: a miss has none; a hit's primitive carries the reported material
    miss = ref[:, 9] < 0
    prim = got[:, 10]
    assert (prim[miss] == rtc.REF_NONE).all(), what
    s = sc.s
    kind, idx = (prim.astype(np.uint32) >> 28).astype(np.int64), (prim & ((1 << 28) - 1)).astype(np.int64)
    mats = np.full(len(rays), -2, np.int64)
    for k, (arr, col) in {1: (_words(s.spheres, s.n_spheres, 8), 6), 2: (_words(s.quads, s.n_quads, 20), 11),
                          6: (_words(s.media, s.n_media, 4), 2)}.items():
        sel = ~miss & (kind == k)
        assert (idx[sel] < len(arr)).all(), what
        mats[sel] = arr[idx[sel], col]
    assert (mats[~miss] == got[~miss, 9]).all(), f"{what}: prim and material disagree"
    assert ((kind[~miss] == 6) == medium[~miss]).all(), f"{what}: MEDIUM prims and the in-medium flag disagree"
    if prim_t:  # no transforms in this scene: the primitive alone gives the same t
        L, t = _ref_lib(), ctypes.c_float()
        for k in np.flatnonzero(~miss):
            assert L.query_ref_prim(ctypes.cast(sc.ptr, ctypes.c_void_p), int(prim[k]), rays[k].ctypes.data, tmin, tmax,
                                    ctypes.byref(t)) == 1, f"{what}: ray {k}: prim {prim[k]:#x} is not hit"
            assert np.float32(t.value).view(np.int32) == got[k, 0], f"{what}: ray {k}: prim {prim[k]:#x} gives another t"


def has_transforms(sc):
    return (sc.features & rtc.FEAT_XFORM) != 0


# ------------------------------------------------------------------------------------ without a GPU
def _host_check(tmp_path, scene_id, tmax, n_lds, naive=False, rng=(0, 0)):
    rays = make_rays(scene_id)
    rp, hp = str(tmp_path / "rays.bin"), str(tmp_path / "hits.bin")
    rays.tofile(rp)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1")
    args = [HOST, str(scene_id), str(WIDTH), rp, hp, "0.001", "inf" if tmax == INF else float(tmax).hex(),
            str(rng[0]), str(rng[1]), str(n_lds)] + (["naive"] if naive else [])
    r = subprocess.run(args, capture_output=True, text=True, env=env, timeout=600, cwd=rtc.substitute_dir())
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert int(r.stdout.split()[0]) == N
    return np.fromfile(hp, np.int32).reshape(N, 12)


@pytest.mark.parametrize("scene_id", SCENES)
def test_query_code_on_host_matches_reference(tmp_path, scene_id):
    """rt_query.h's per-lane code with the emulated refill rounds (three waves sharing the counter, 37
    entries read through the LDS copy), every tmax; then the one-ray-per-thread form."""
    sc = scene(scene_id)
    for tmax in tmax_values(scene_id):
        got = _host_check(tmp_path, scene_id, tmax, 37)
        check_hits(sc, make_rays(scene_id), got, reference(scene_id, tmax), f"scene {scene_id} tmax {tmax}", tmax=tmax,
                   prim_t=not has_transforms(sc))
    tmax = tmax_values(scene_id)[2]
    got = _host_check(tmp_path, scene_id, tmax, 0, naive=True)
    check_hits(sc, make_rays(scene_id), got, reference(scene_id, tmax), f"scene {scene_id} naive", tmax=tmax)


def test_query_batches_are_not_vacuous():
    """Scene 7 at its default density gives medium hits and misses, and every finite bound cuts hits off."""
    ref = reference(7)
    medium = (ref[:, 11] & rtc.HIT_IN_MEDIUM) != 0
    miss = ref[:, 9] < 0
    assert medium.sum() >= 20 and miss.sum() >= 20, (medium.sum(), miss.sum())
    for sid in SCENES:
        full = reference(sid)
        for tmax in tmax_values(sid)[1:]:
            cut = reference(sid, tmax)
            assert ((cut[:, 9] < 0) & (full[:, 9] >= 0)).any(), f"scene {sid}: tmax {tmax} cuts nothing off"
            t = cut[:, 0].view(np.float32)
            assert (t[cut[:, 9] >= 0] <= np.float32(tmax)).all()
        assert len(set(tmax_values(sid))) == 4


def test_query_reference_is_independent_of_batch_order():
    """The checker itself: ray k's stream depends on rng_seq + k only."""
    sc, rays = scene(7), make_rays(7)
    a = query_ref(sc, rays[100:200], 1e-3, INF, (5, 100))
    b = query_ref(sc, rays, 1e-3, INF, (5, 0))[100:200]
    assert (a == b).all()


def test_hits_views_on_numpy():
    raw = np.arange(24, dtype=np.int32).reshape(2, 12)
    raw[:, 11] = (rtc.HIT_FRONT_FACE | rtc.HIT_IN_MEDIUM, rtc.HIT_FRONT_FACE)
    h = rtc.Hits(raw)
    assert len(h) == 2 and h.p.shape == (2, 3) and h.normal.shape == (2, 3) and h.uv.shape == (2, 2)
    assert h.t.dtype == np.float32 and h.t.view(np.int32).tolist() == [0, 12]
    assert h.material.tolist() == [9, 21] and h.prim.tolist() == [10, 22]
    assert h.front.tolist() == [True, True] and h.in_medium.tolist() == [True, False]


# ------------------------------------------------------------------------------------ on the GPU
def _trace(ds, rays, tmax=INF, rng=(0, 0), tmin=1e-3):
    import torch

    r = torch.from_numpy(np.array(rays, np.float32)).to("cuda:0")
    h = ds.trace_rays(r, tmin, tmax, rng, torch.cuda.current_stream(0).cuda_stream)
    torch.cuda.synchronize()
    return h.raw.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("scene_id", SCENES)
def test_gpu_query_matches_reference(scene_id):
    sc = scene(scene_id)
    ds = rtc.DeviceScene(sc, 0)
    try:
        for tmax in tmax_values(scene_id):
            got = _trace(ds, make_rays(scene_id), tmax)
            check_hits(sc, make_rays(scene_id), got, reference(scene_id, tmax), f"scene {scene_id} tmax {tmax}",
                       tmax=tmax, prim_t=not has_transforms(sc))
    finally:
        ds.close()


def _diag_scene(monkeypatch, scene_id, naive, **env):
    """A device scene of the diagnostic build: the persistent kernel (naive = "0") or the naive launch."""
    monkeypatch.setenv("RT_QUERY_NAIVE", naive)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with rtc.use_diag():
        return rtc.DeviceScene(rtc.Scene.preset(scene_id, WIDTH, 1, 1), 0)


@pytest.mark.gpu
@pytest.mark.parametrize("naive", ["0", "1"])
@pytest.mark.parametrize("scene_id", SCENES)
def test_gpu_query_diag_variants_agree(scene_id, naive, monkeypatch):
    """The diagnostic build's persistent kernel (RT_QUERY_NAIVE=0) and its one-ray-per-thread launch
    (RT_QUERY_NAIVE=1) against the reference and, record for record including prim, against the library."""
    sc = scene(scene_id)
    tmax = tmax_values(scene_id)[2]
    ds = rtc.DeviceScene(sc, 0)
    dn = _diag_scene(monkeypatch, scene_id, naive, RT_GEN_PRE="0")  # (RT_GEN_PRE=0 must not disable queries)
    try:
        for tm in (INF, tmax):
            a, b = _trace(ds, make_rays(scene_id), tm), _trace(dn, make_rays(scene_id), tm)
            check_hits(sc, make_rays(scene_id), b, reference(scene_id, tm), f"scene {scene_id} naive={naive} tmax {tm}", tmax=tm)
            assert (a == b).all(), f"scene {scene_id}: {(a != b).any(axis=1).sum()} records differ between the kernels"
    finally:
        ds.close()
        dn.close()


@pytest.mark.gpu
@pytest.mark.parametrize("persistent", [False, True])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_gpu_query_small_batches(n, persistent, monkeypatch):
    sc = scene(6)
    ds = _diag_scene(monkeypatch, 6, "0") if persistent else rtc.DeviceScene(sc, 0)
    try:
        got = _trace(ds, make_rays(6)[:n])
        assert got.shape == (n, 12)
        if n:
            check_hits(sc, make_rays(6)[:n], got, reference(6)[:n], f"n = {n}")
    finally:
        ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("persistent", [False, True])
@pytest.mark.parametrize("scene_id", [1, 5])
def test_gpu_query_permuted_rays_give_permuted_hits(scene_id, persistent, monkeypatch):
    ds = _diag_scene(monkeypatch, scene_id, "0") if persistent else rtc.DeviceScene(scene(scene_id), 0)
    try:
        rays = make_rays(scene_id)
        perm = np.random.default_rng(7).permutation(N)
        a, b = _trace(ds, rays), _trace(ds, rays[perm])
        assert (a[perm] == b).all()
    finally:
        ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("persistent", [False, True])
def test_gpu_query_between_two_render_launches(manifest, persistent, monkeypatch):
    """A query queued between two row launches on the same scene and stream leaves the frame equal to the
    golden: the query shares no scratch with the renders (the persistent kernel has a work counter of its own)."""
    import torch

    e = manifest["renders"]["s5_200x112_16spp_d50"]
    sc = rtc.Scene.preset(5, 200, 16, 50)
    if persistent:
        monkeypatch.setenv("RT_QUERY_NAIVE", "0")
    with rtc.use_diag(persistent):
        ds = rtc.DeviceScene(sc, 0)
    try:
        st = torch.cuda.current_stream(0).cuda_stream
        frame = torch.zeros((sc.height, sc.width, 3), dtype=torch.uint8, device="cuda:0")
        rays = torch.from_numpy(np.array(make_rays(5))).to("cuda:0")
        half = sc.height // 2
        ds.render_rows_async(0, 1, half, frame.data_ptr(), st)
        hits = ds.trace_rays(rays, stream_ptr=st)
        ds.render_rows_async(half, 1, sc.height - half, frame[half:].data_ptr(), st)
        torch.cuda.synchronize()
        ds.check()
        assert (frame.cpu().numpy() == golden_image(e)).all()
        check_hits(scene(5), make_rays(5), hits.raw.cpu().numpy(), reference(5), "between two launches")
    finally:
        ds.close()


@pytest.mark.gpu
def test_gpu_query_on_book1_scene_then_render(manifest):
    """A Book-1 scene builds no preorder for its render path: the first query makes the device copy, and
    the render after it is the golden frame."""
    import torch

    e = manifest["renders"]["s1_300x168_16spp_d50"]
    sc = rtc.Scene.preset(1, 300, 16, 50)
    ds = rtc.DeviceScene(sc, 0)
    try:
        assert "book1" in ds.kernel_name
        rays = make_rays(1)  # (the scene's objects do not depend on the image size)
        got = _trace(ds, rays)
        check_hits(sc, rays, got, reference(1), "book-1 scene", prim_t=True)
        frame = torch.empty((sc.height, sc.width, 3), dtype=torch.uint8, device="cuda:0")
        ds.render_rows_async(0, 1, sc.height, frame.data_ptr(), torch.cuda.current_stream(0).cuda_stream)
        torch.cuda.synchronize()
        ds.check()
        assert (frame.cpu().numpy() == golden_image(e)).all()
        assert (_trace(ds, rays) == got).all()
    finally:
        ds.close()


@pytest.mark.gpu
def test_gpu_query_host_buffers_equal_async():
    ds = rtc.DeviceScene(scene(7), 0)
    try:
        rays = make_rays(7)
        h = rtc.trace_rays_host(ds, rays, 1e-3, tmax_values(7)[2], (3, 11))
        assert (h.raw == _trace(ds, rays, tmax_values(7)[2], (3, 11))).all()
        assert h.t.dtype == np.float32 and h.in_medium.any() and not h.front[h.prim == rtc.REF_NONE].any()
        assert len(rtc.trace_rays_host(ds, rays[:0])) == 0
    finally:
        ds.close()


@pytest.mark.gpu
def test_gpu_query_rejects_bad_arguments():
    import torch

    ds = rtc.DeviceScene(scene(1), 0)
    L = rtc.lib()
    rays = torch.from_numpy(np.array(make_rays(1)[:8])).to("cuda:0")
    hits = torch.empty((8, 12), dtype=torch.int32, device="cuda:0")
    ok = rtc.RtQueryParams(1e-3, INF, 0, 0)

    def call(h, r, n, prm, out):
        rc = L.rt_trace_rays_async(h, r, n, prm, out, None)
        return rc, rtc.last_error(L)

    try:
        cases = {"NULL scene": (None, rays.data_ptr(), 8, ctypes.byref(ok), hits.data_ptr()),
                 "NULL rays": (ds._h, None, 8, ctypes.byref(ok), hits.data_ptr()),
                 "NULL hits": (ds._h, rays.data_ptr(), 8, ctypes.byref(ok), None),
                 "NULL params": (ds._h, rays.data_ptr(), 8, None, hits.data_ptr()),
                 "n < 0": (ds._h, rays.data_ptr(), -1, ctypes.byref(ok), hits.data_ptr()),
                 "tmin NaN": (ds._h, rays.data_ptr(), 8, ctypes.byref(rtc.RtQueryParams(float("nan"), 1.0, 0, 0)),
                              hits.data_ptr()),
                 "tmax NaN": (ds._h, rays.data_ptr(), 8, ctypes.byref(rtc.RtQueryParams(0.0, float("nan"), 0, 0)),
                              hits.data_ptr()),
                 "tmin > tmax": (ds._h, rays.data_ptr(), 8, ctypes.byref(rtc.RtQueryParams(2.0, 1.0, 0, 0)),
                                 hits.data_ptr())}
        for what, args in cases.items():
            rc, msg = call(*args)
            assert rc == -1 and msg, what
        assert L.rt_trace_rays(ds._h, None, 8, ctypes.byref(ok), None) == -1 and rtc.last_error(L)
        assert L.rt_trace_rays_async(ds._h, None, 0, ctypes.byref(ok), None, None) == 0  # n == 0: no launch
        with pytest.raises(ValueError):
            ds.trace_rays(rays[:, :5])
        with pytest.raises(rtc.RtcError):
            ds.trace_rays(rays, tmin=2.0, tmax=1.0)
        assert (_trace(ds, make_rays(1)[:8]) == reference(1)[:8])[:, :10].all()  # the scene still answers
    finally:
        ds.close()


@pytest.mark.gpu
def test_gpu_query_rng_changes_only_medium_hits():
    sc, rays = scene(7), make_rays(7)
    ds = rtc.DeviceScene(sc, 0)
    try:
        a, b = _trace(ds, rays, rng=(0, 0)), _trace(ds, rays, rng=(12345, 77))
        check_hits(sc, rays, b, query_ref(sc, rays, 1e-3, INF, (12345, 77)), "rng (12345, 77)")
        differ = (a != b).any(axis=1)
        medium = ((a[:, 11] | b[:, 11]) & rtc.HIT_IN_MEDIUM) != 0
        assert differ.any() and not (differ & ~medium).any()
    finally:
        ds.close()
