"""Parity of the gfx950 render path (through the C ABI) with the reference.

Bar: bit-exact.  Every pixel of every frame must equal the reference CPU render built from the
reference's own sources (golden fixtures) and the oracle restatement on the same inputs.
"""
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import pyoracle
import rtc
from conftest import ROOT, golden_image

pytestmark = pytest.mark.gpu


def _check(img, ref, what):
    bad = (img != ref).any(axis=-1)
    if bad.any():
        y, x = np.argwhere(bad)[0]
        pytest.fail(f"{what}: {bad.sum()} / {bad.size} pixels differ; first at (x={x}, y={y}): "
                    f"gpu={img[y, x].tolist()} ref={ref[y, x].tolist()}")


def test_device_visible():
    assert rtc.device_count() >= 1, "no HIP device: this library has no CPU fallback"


@pytest.mark.parametrize("name", [
    "s0_400x225_10spp_d10", "s0_400x225_100spp_d50", "s1_300x168_16spp_d50", "s2_200x112_8spp_d50",
    "s3_200x112_8spp_d50", "s4_200x112_8spp_d50", "s5_200x112_16spp_d50", "s6_200x200_16spp_d50",
    "s7_200x200_8spp_d50"])
def test_gpu_matches_reference_render(manifest, name):
    e = manifest["renders"][name]
    sc = rtc.Scene.preset(e["scene"], e["width"], e["spp"], e["depth"])
    img = rtc.render(sc, n_gpus=1)
    _check(img, golden_image(e), name)


@pytest.mark.parametrize("name", ["s1_1200x675_10spp_d50", "s7_400x400_16spp_d50"])
def test_gpu_matches_reference_sha(manifest, name):
    e = manifest["renders"][name]
    img = rtc.render(rtc.Scene.preset(e["scene"], e["width"], e["spp"], e["depth"]))
    assert hashlib.sha256(img.tobytes()).hexdigest() == e["sha256"], name


def test_gpu_north_star_frame_pixel_identical(manifest):
    """Book-1 final scene, 1200x675, 1000 spp, depth 50: the headline configuration."""
    e = manifest["renders"].get("s1_1200x675_1000spp_d50")
    if e is None:
        pytest.skip("north-star golden not generated (make_golden.py --big)")
    img = rtc.render(rtc.Scene.preset(1, 1200, 1000, 50))
    got = hashlib.sha256(img.tobytes()).hexdigest()
    if got != e["sha256"]:
        bad = [c for c, h in e["crops"].items() if hashlib.sha256(
            img[int(c.split(",")[1]):int(c.split(",")[1]) + 32, int(c.split(",")[0]):int(c.split(",")[0]) + 32]
            .tobytes()).hexdigest() != h]
        pytest.fail(f"full-frame sha mismatch; crops differing: {bad}")


def test_gpu_headline_scene_other_resolution(manifest):
    """The headline scene at another resolution (800x450, 1000 spp: 0.44 M pixels, which the planner runs
    in the class of an N = 2 share) is the reference frame (r06 generalisation check)."""
    e = manifest["renders"].get("s1_800x450_1000spp_d50")
    if e is None:
        pytest.skip("golden not generated (make_golden.py --only s1_800x450_1000spp_d50)")
    img = rtc.render(rtc.Scene.preset(1, 800, 1000, 50))
    assert hashlib.sha256(img.tobytes()).hexdigest() == e["sha256"]


@pytest.mark.parametrize("world", [8, 4, 2])
def test_gpu_north_star_rank_shares_reassemble(manifest, world):
    """BASELINE config 4 (the north-star frame over 8 GPUs, rows j % 8) rehearsed on one device:
    every rank's share rendered as its own launch (the multi-GPU bench's per-rank call), then
    reassembled: the frame's sha must equal the reference render's."""
    import torch

    e = manifest["renders"].get("s1_1200x675_1000spp_d50")
    if e is None:
        pytest.skip("north-star golden not generated (make_golden.py --big)")
    sc = rtc.Scene.preset(1, 1200, 1000, 50)
    ds = rtc.DeviceScene(sc, 0)
    stream = torch.cuda.current_stream(0)
    parts = []
    for rank in range(world):
        row0, stride, n = rtc.rows_of(sc.height, rank, world)
        buf = torch.empty((n, sc.width, 3), dtype=torch.uint8, device="cuda:0")
        ds.render_rows_async(row0, stride, n, buf.data_ptr(), stream.cuda_stream)
        torch.cuda.synchronize()
        ds.check()
        parts.append(buf.cpu().numpy())
    ds.close()
    frame = rtc.assemble_frame(parts, sc.height, world)
    assert hashlib.sha256(frame.tobytes()).hexdigest() == e["sha256"], f"{world} rank shares"


def test_gpu_scene7_config5_full_size(manifest):
    """BASELINE config 5 at full size: scene 7 (Book-2 final), 1000x1000, 1000 spp, depth 50."""
    e = manifest["renders"].get("s7_1000x1000_1000spp_d50")
    if e is None:
        pytest.skip("config-5 golden not generated (make_golden.py --big)")
    img = rtc.render(rtc.Scene.preset(7, 1000, 1000, 50))
    got = hashlib.sha256(img.tobytes()).hexdigest()
    if got != e["sha256"]:
        bad = [c for c, h in e["crops"].items() if hashlib.sha256(
            img[int(c.split(",")[1]):int(c.split(",")[1]) + 32, int(c.split(",")[0]):int(c.split(",")[0]) + 32]
            .tobytes()).hexdigest() != h]
        pytest.fail(f"config-5 full-frame sha mismatch; crops differing: {bad}")


@pytest.mark.parametrize("scene,width,spp,depth", [
    (0, 97, 7, 3), (1, 211, 5, 50), (1, 64, 2, 1), (2, 150, 4, 7), (4, 120, 3, 50), (5, 131, 9, 50),
    (6, 90, 6, 50), (7, 128, 4, 50), (3, 100, 3, 2), (1, 2, 11, 50)])
def test_gpu_matches_oracle(scene, width, spp, depth):
    """Odd sizes, shallow depths and every scene kind against the CPU restatement."""
    sc = rtc.Scene.preset(scene, width, spp, depth)
    _check(rtc.render(sc), pyoracle.render(sc), f"scene {scene} {width}px {spp}spp d{depth}")


def test_gpu_depth_zero_is_black():
    sc = rtc.Scene.preset(1, 64, 2, 1)
    sc.s.camera.max_depth = 0
    assert rtc.render(sc).max() == 0


def test_gpu_interleaved_rows_on_one_device(manifest):
    """rt_render_rows_async with row stride (the multi-GPU partition) writes the frame's rows."""
    import torch

    e = manifest["renders"]["s1_300x168_16spp_d50"]
    ref = golden_image(e)
    sc = rtc.Scene.preset(1, 300, 16, 50)
    ds = rtc.DeviceScene(sc, 0)
    for world in (2, 3, 8):
        for rank in range(world):
            row0, stride, n = rtc.rows_of(sc.height, rank, world)
            buf = torch.empty((n, sc.width, 3), dtype=torch.uint8, device="cuda:0")
            stream = torch.cuda.current_stream(0)
            ds.render_rows_async(row0, stride, n, buf.data_ptr(), stream.cuda_stream)
            torch.cuda.synchronize()
            _check(buf.cpu().numpy(), ref[row0::stride][:n], f"rows {rank}/{world}")
    ds.close()


@pytest.mark.parametrize("scene,width,spp", [(1, 300, 128), (5, 200, 64), (1, 300, 16)])
def test_gpu_launches_on_two_streams_serialise(scene, width, spp):
    """Launches on one scene share its scratch (rt_hip.h): two row bands queued back to back on two
    streams, with no host synchronisation between them, must give the rows of a one-stream render
    (chain render, general path and lane kernel)."""
    import torch

    sc = rtc.Scene.preset(scene, width, spp, 50)
    ds = rtc.DeviceScene(sc, 0)
    full = torch.empty((sc.height, sc.width, 3), dtype=torch.uint8, device="cuda:0")
    ds.render_rows_async(0, 1, sc.height, full.data_ptr(), torch.cuda.current_stream(0).cuda_stream)
    torch.cuda.synchronize()
    ref = full.cpu().numpy()
    s1, s2 = torch.cuda.Stream(0), torch.cuda.Stream(0)
    half = sc.height // 2
    a = torch.empty((half, sc.width, 3), dtype=torch.uint8, device="cuda:0")
    b = torch.empty((sc.height - half, sc.width, 3), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    for _ in range(2):
        ds.render_rows_async(0, 1, half, a.data_ptr(), s1.cuda_stream)
        ds.render_rows_async(half, 1, sc.height - half, b.data_ptr(), s2.cuda_stream)
    torch.cuda.synchronize()
    ds.close()
    _check(a.cpu().numpy(), ref[:half], f"scene {scene} band 0 on stream 1")
    _check(b.cpu().numpy(), ref[half:], f"scene {scene} band 1 on stream 2")


def test_gpu_rejects_out_of_range_rows():
    sc = rtc.Scene.preset(0, 40, 1, 1)
    ds = rtc.DeviceScene(sc, 0)
    with pytest.raises(rtc.RtcError):
        ds.render_rows_async(0, 1, sc.height + 1, 1, 0)
    ds.close()


def _run_cli(exe, args, cwd):
    env = dict(os.environ, RT_NUM_GPUS="1")
    r = subprocess.run([exe, *args], cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(os.path.join(cwd, "output.tiff"), "rb").read(), r.stderr


def test_dropin_reference_main_renders_identical_tiff(manifest, tmp_path):
    """The reference's own src/main.c, compiled unchanged against include/ and linked to
    librtc_amd.so (oracle/_ref/ref_main_dropin), writes the reference's TIFF byte for byte."""
    exe = pyoracle.REF_DROPIN
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/ref_main_dropin not built (needs /root/reference at build time)")
    data, err = _run_cli(exe, ["0", "400", "1", "_"], str(tmp_path))  # argc quirk: 4th arg needed for spp
    assert "Book 1: Metal and Lambertian" in err and "Took" in err
    e = manifest["renders"]["s0_400x225_10spp_d10"]
    sc = rtc.Scene.preset(0, 400, 1, 50)
    img = pyoracle.render(sc)
    assert data[168:] == img.tobytes()
    assert len(data) == 168 + e["width"] * e["height"] * 3


def test_cli_rt_main_matches_golden(manifest, tmp_path):
    exe = os.path.join(ROOT, "ray-tracing-c_amd", "rt_main")
    env_depth = "10"
    os.environ["RT_MAX_DEPTH"] = env_depth
    try:
        data, err = _run_cli(exe, ["0", "400", "10", "_"], str(tmp_path))
    finally:
        del os.environ["RT_MAX_DEPTH"]
    e = manifest["renders"]["s0_400x225_10spp_d10"]
    assert hashlib.sha256(data[168:]).hexdigest() == e["sha256"]
    assert data[:168] == open(os.path.join(ROOT, "tests", "golden", "tiff_header.bin"), "rb").read()


# Tests that select a path or force a fallback by RT_* switches use the diagnostic build
# (librtc_amd_diag.so, -DRT_DIAG: the product library reads only the planner parameters).
CHAIN = {"RT_MODE": "chain", "RT_LPT_SPP": "1", "RT_CHAIN_MIN_SEG": "4"}
SPLIT = {**CHAIN, "RT_CHAIN_BETA": "0.001"}  # every pixel split as far as allowed


@pytest.mark.parametrize("env", [
    {},                                                       # the default plan (chain at 100 spp, lanes at 16)
    {"RT_MODE": "lane"},                                      # the lane kernel (low spp, small launches)
    {"RT_BOOK1_LDS": "0", "RT_MODE": "lane"},                 # scenes whose items exceed 64 KiB: global memory
    {**SPLIT, "RT_BOOK1_LDS": "0"},                           #   ... chain render on them (lanes only)
    CHAIN, SPLIT,                                             # the chain render, planned / fully split
    {**SPLIT, "RT_CHAIN_KMAX": "1"},                          # every split pixel on whole waves
    {**SPLIT, "RT_CHAIN_KMAX": "1", "RT_BF_CUTS": "0"},       #   ... their candidate trace over every leaf
    {**SPLIT, "RT_CHAIN_KMAX": "1", "RT_BF": "0"},            #   ... and the exact whole-wave scan
    {**SPLIT, "RT_CHAIN_MARGIN": "1.0", "RT_CHAIN_SLACK": "1"},  # lists that fill up: continuations
    {**SPLIT, "RT_CHAIN_MB": "1"},                            # out of records: pixels stay whole
    {**CHAIN, "RT_CHAIN_OCC": "3"}, {**CHAIN, "RT_CHAIN_OCC": "5"},  # both chain kernel occupancies
    {"RT_BOOK1": "0"},                                        # the general kernel on Book-1 scenes
])
@pytest.mark.parametrize("name", ["s0_400x225_100spp_d50", "s1_300x168_16spp_d50"])
def test_book1_shipped_paths_reproduce_reference(manifest, name, env, monkeypatch):
    """Every path the product takes for Book-1 scenes -- lane or chain kernel, LDS or global-memory
    items, split / whole-wave / continuation / unsplit-fallback items, both occupancies -- and the
    general kernel on the same scenes, forced on small goldens: each must reproduce the reference frame."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    e = manifest["renders"][name]
    with rtc.use_diag():
        img = rtc.render(rtc.Scene.preset(e["scene"], e["width"], e["spp"], e["depth"]))
    _check(img, golden_image(e), f"{name} {env}")


@pytest.mark.parametrize("scene,width,spp,depth", [(1, 96, 6, 65), (1, 80, 4, 100), (5, 64, 4, 100), (7, 48, 2, 120)])
def test_gpu_depth_beyond_64_matches_oracle(scene, width, spp, depth):
    """max_depth > 64: the deep kernel (global-memory path records) against the oracle."""
    sc = rtc.Scene.preset(scene, width, spp, depth)
    _check(rtc.render(sc), pyoracle.render(sc), f"scene {scene} depth {depth}")


def test_book1_deep_paths_spill(monkeypatch):
    """max_depth 64 with a glass-heavy view: paths longer than the register record spill to HBM."""
    sc = rtc.Scene.preset(1, 160, 24, 64)
    _check(rtc.render(sc), pyoracle.render(sc), "scene 1 depth 64")


@pytest.mark.parametrize("env", [{}, {"RT_CHAIN_BETA": "0.002"}, {"RT_CHAIN_BETA": "0.002", "RT_CHAIN_KMAX": "64"},
                                 {"RT_CHAIN_BETA": "0.002", "RT_CHAIN_MARGIN": "1.0", "RT_CHAIN_SLACK": "1"},
                                 {"RT_CHAIN_OCC": "3"}, {"RT_CHAIN_OCC": "5", "RT_CHAIN_BETA": "0.002"},
                                 {"RT_CHAIN_BETA": "0.002", "RT_CHAIN_COVER": "2", "RT_CHAIN_COVER_K": "2"},
                                 {"RT_CHAIN_BETA": "0.002", "RT_CHAIN_OCC": "3", "RT_CHAIN_HEAVY": "3",
                                  "RT_CHAIN_HEAVY_K": "2"}])
def test_chain_render_north_star_scene(manifest, env, monkeypatch):
    """Chain render (rt_book1.h: ChainPx) forced on the Book-1 final scene at full size: pixel
    streams cut into segments, chains coupling on equal stream offsets, the fold and the
    continuations must reproduce the reference frame bit for bit."""
    monkeypatch.setenv("RT_MODE", "chain")
    monkeypatch.setenv("RT_LPT_SPP", "2")
    monkeypatch.setenv("RT_CHAIN_MIN_SEG", "2")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    e = manifest["renders"]["s1_1200x675_10spp_d50"]
    with rtc.use_diag():
        img = rtc.render(rtc.Scene.preset(e["scene"], e["width"], e["spp"], e["depth"]))
    assert hashlib.sha256(img.tobytes()).hexdigest() == e["sha256"], env


def test_chain_record_arena_clean_across_launches(manifest, monkeypatch):
    """The record arena is clean between chain launches only because each launch's cost pre-pass sets
    the previous launch's reservation back (rt_book1.h: clean_records) and a fresh arena's records are
    filled only as far as a launch reserves past the clean high-water mark (chain_fill_kernel, r06):
    launches of growing and shrinking reservations on one device scene -- two rank shares of a fresh
    arena, the whole frame (growing past them), eight and two rank shares, the whole frame again -- must
    each reproduce the reference rows."""
    import torch

    monkeypatch.setenv("RT_MODE", "chain")
    monkeypatch.setenv("RT_LPT_SPP", "2")
    monkeypatch.setenv("RT_CHAIN_MIN_SEG", "2")
    monkeypatch.setenv("RT_CHAIN_BETA", "0.002")
    e = manifest["renders"]["s1_300x168_16spp_d50"]
    ref = golden_image(e)
    with rtc.use_diag():
        sc = rtc.Scene.preset(e["scene"], e["width"], e["spp"], e["depth"])
        ds = rtc.DeviceScene(sc, 0)
    stream = torch.cuda.current_stream(0)
    for world, ranks in ((8, [7, 0]), (1, [0]), (8, range(8)), (2, range(2)), (1, [0]), (8, [7, 0])):
        for rank in ranks:
            row0, stride, n = rtc.rows_of(sc.height, rank, world)
            buf = torch.empty((n, sc.width, 3), dtype=torch.uint8, device="cuda:0")
            ds.render_rows_async(row0, stride, n, buf.data_ptr(), stream.cuda_stream)
            torch.cuda.synchronize()
            ds.check()
            _check(buf.cpu().numpy(), ref[row0::stride][:n], f"chain launch rows {rank}/{world}")
    ds.close()


@pytest.mark.parametrize("env", [{"RT_GEN_BIG": "0"}, {"RT_GEN_BIG": "0", "RT_GEN_LDS": "0"},
                                 {"RT_GEN_BIG": "0", "RT_GEN_LDS": "7"}, {"RT_GEN_PERLIN_LDS": "0"}])
@pytest.mark.parametrize("name", ["s5_200x112_16spp_d50", "s6_200x200_16spp_d50", "s7_200x200_8spp_d50"])
def test_general_path_shipped_variants(manifest, name, env, monkeypatch):
    """The general kernel as it ships for scenes whose preorder exceeds one workgroup's LDS (256-thread
    workgroups, the preorder's top staged in LDS or none of it) and without the Perlin tables in LDS:
    each must reproduce the reference frames (transforms, media, lights).  (The default, whole
    preorder in one 768-thread workgroup's LDS, is test_gpu_matches_reference_render.)"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    e = manifest["renders"][name]
    with rtc.use_diag():
        img = rtc.render(rtc.Scene.preset(e["scene"], e["width"], e["spp"], e["depth"]))
    _check(img, golden_image(e), f"{name} {env}")


@pytest.mark.parametrize("env", [{"RT_GEN_PRE": "0"}, {"RT_GEN_BATCH": "0"}, {"RT_GEN_BATCH": "1"}, {"RT_GEN_BATCH": "64"},
                                 {"RT_GEN_FLAT": "1"}, {"RT_GEN_RARE": "1"}, {"RT_GEN_STEPS": "3"}, {"RT_LPT_SPP": "2"},
                                 {"RT_LPT_SPP": "2", "RT_LPT": "0"}])
def test_general_path_diag_switches(manifest, env, monkeypatch):
    """The diagnostic build's remaining A/B switches of the general kernel: no preorder
    (stack traversal), unbatched / one-lane / full-wave shading batches, no extra box entries per step,
    rare actions at once, short trace iterations, the longest-first pre-pass on (2 spp) or off -- each changes only the
    schedule, so scene 7 must still reproduce the reference frame."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    e = manifest["renders"]["s7_200x200_8spp_d50"]
    with rtc.use_diag():
        img = rtc.render(rtc.Scene.preset(e["scene"], e["width"], e["spp"], e["depth"]))
    _check(img, golden_image(e), f"s7 {env}")


def test_bench_two_rank_launch_reassembles_reference_frame():
    """bench.py's N-rank path (torch.distributed.run, rows j % N, gather, parity) run as 2 ranks on
    this box's GPU(s) (RT_BENCH_SHARE_DEVICE=1: gloo for the reduction and the gather), on the
    north-star scene at 10 spp: the gathered frame must be the reference render (golden
    s1_1200x675_10spp_d50)."""
    import json
    import sys
    env = dict(os.environ, RT_BENCH_SHARE_DEVICE="1", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", "29533", os.path.join(ROOT, "bench.py"),
           "--gpus", "2", "--steps", "1", "--warmup", "0", "--spp", "10", "--full", "--no-cpu-baseline"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["config"]["partition"] == "rows j % 2"
    assert line["parity"]["golden"] == "s1_1200x675_10spp_d50"
    assert line["parity"]["pixel_identical_to_reference"] is True
    assert line["parity"]["max_abs_pixel_diff"] == 0


def test_record_arena_grows_for_async_launches(monkeypatch):
    """A plan that wants more records than the arena's bound holds keeps its excess pixels whole (exact, but a
    whole 1000-sample chain per lane: ~3x slower).  rt_render_share grows the next arena from a synchronous
    read-back; rt_render_rows_async (DeviceScene, bench.py) from the plan's reservation copied to pinned memory
    and read by the next launch once it has landed.  Forced here with a tail-shaping alpha of 1.0 on an N = 4
    share of the headline frame (its plan wants ~795 M records against a bound of ~739 M): the launches after the
    first must run on a grown arena -- several times faster -- with the same rows."""
    import torch

    monkeypatch.setenv("RT_CHAIN_ALPHA", "1.0")
    with rtc.use_diag():
        sc = rtc.Scene.preset(1, 1200, 1000, 50)
        ds = rtc.DeviceScene(sc, 0)
    stream = torch.cuda.current_stream(0)
    row0, stride, n = rtc.rows_of(sc.height, 0, 4)
    ms, rows = [], []
    for _ in range(3):
        buf = torch.empty((n, sc.width, 3), dtype=torch.uint8, device="cuda:0")
        ds.render_rows_async(row0, stride, n, buf.data_ptr(), stream.cuda_stream)
        torch.cuda.synchronize()
        ds.check()
        ms.append(ds.last_launch_ms())
        rows.append(buf.cpu().numpy())
    ds.close()
    assert all((r == rows[0]).all() for r in rows[1:])
    assert ms[2] < 0.6 * ms[0], ms


# Tail migration (rt_book1.h: MigRec) forced onto every wave that runs out of work: any wave with
# live lanes and no items left hands them to helpers, every finished wave stays a helper.
MIGRATE = {**CHAIN, "RT_CHAIN_BETA": "0.001", "RT_MIG_LIVE": "63", "RT_MIG_IDLE": "0", "RT_MIG_HELP": "100"}


@pytest.mark.parametrize("wait_us", ["0", "1", "200"])
def test_migration_helpers_leaving_early_lose_no_work(manifest, wait_us, monkeypatch):
    """Helpers that give up waiting at once (RT_MIG_WAIT_US ~ 0) must not strand migrated items: a
    helper leaves only by taking back an unclaimed credit.  The result must be the exact frame (or a
    loud error), never a wrong image with status 0 (VERDICT r02 / ADVICE r02: rt_book1.h mig_help)."""
    for k, v in {**MIGRATE, "RT_MIG_WAIT_US": wait_us}.items():
        monkeypatch.setenv(k, v)
    e = manifest["renders"]["s1_300x168_16spp_d50"]
    with rtc.use_diag():
        img = rtc.render(rtc.Scene.preset(e["scene"], e["width"], e["spp"], e["depth"]))
    _check(img, golden_image(e), f"migration, helpers wait {wait_us} us")


def test_lost_work_item_is_reported_not_rendered_silently(manifest, monkeypatch):
    """Fault injection: a helper drops a migrated item unrun.  The completion check after the chain
    launch (chain_check_kernel) must turn that into an error from rt_render -- Camera_render then
    aborts -- instead of a frame with an unwritten pixel and status 0 (SURVEY §8b "Errors")."""
    for k, v in {**MIGRATE, "RT_MIG_WAIT_US": "2000", "RT_FAULT_MIG_DROP": "1"}.items():
        monkeypatch.setenv(k, v)
    e = manifest["renders"]["s1_300x168_16spp_d50"]
    with rtc.use_diag():
        with pytest.raises(rtc.RtcError, match="never finished"):
            rtc.render(rtc.Scene.preset(e["scene"], e["width"], e["spp"], e["depth"]))
        # the status is per scene and cleared by the check: a clean render afterwards succeeds
        monkeypatch.delenv("RT_FAULT_MIG_DROP")
        img = rtc.render(rtc.Scene.preset(e["scene"], e["width"], e["spp"], e["depth"]))
    _check(img, golden_image(e), "after the fault")
    # the product library has no fault injection: the same variables render the exact frame
    monkeypatch.setenv("RT_FAULT_MIG_DROP", "1")
    img = rtc.render(rtc.Scene.preset(e["scene"], e["width"], e["spp"], e["depth"]))
    _check(img, golden_image(e), "product library ignores RT_FAULT_MIG_DROP")


def test_rehearsed_eight_device_render_threads(manifest, monkeypatch):
    """rt_render's multi-device path (one host thread, device scene, stream and D2H per share, error
    aggregation) driven with 8 shares on this box's GPU(s) (RT_REHEARSE_DEVICES=8: share g on
    device g % count): the north-star scene at 10 spp must be the reference frame."""
    monkeypatch.setenv("RT_REHEARSE_DEVICES", "8")
    e = manifest["renders"]["s1_1200x675_10spp_d50"]
    img = rtc.render(rtc.Scene.preset(1, 1200, 10, 50), n_gpus=0)
    assert hashlib.sha256(img.tobytes()).hexdigest() == e["sha256"]
    img = rtc.render(rtc.Scene.preset(1, 1200, 10, 50), n_gpus=3)  # uneven row counts per share
    assert hashlib.sha256(img.tobytes()).hexdigest() == e["sha256"]


def test_rehearsed_eight_device_north_star_frame(manifest, monkeypatch):
    """BASELINE config 4 through the product's own multi-device path: the full 1000-spp north-star
    frame rendered by rt_render as 8 concurrent shares (RT_REHEARSE_DEVICES=8) is the reference's."""
    e = manifest["renders"].get("s1_1200x675_1000spp_d50")
    if e is None:
        pytest.skip("north-star golden not generated (make_golden.py --big)")
    monkeypatch.setenv("RT_REHEARSE_DEVICES", "8")
    img = rtc.render(rtc.Scene.preset(1, 1200, 1000, 50), n_gpus=8)
    assert hashlib.sha256(img.tobytes()).hexdigest() == e["sha256"]


def test_dropin_reference_main_on_eight_rehearsed_devices(manifest, tmp_path):
    """The reference's own src/main.c (the single caller of Camera_render, src/main.c:336) linked to
    this library, with RT_NUM_GPUS=8 on 8 rehearsed devices: byte-identical TIFF pixels."""
    exe = pyoracle.REF_DROPIN
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/ref_main_dropin not built (needs /root/reference at build time)")
    env = dict(os.environ, RT_NUM_GPUS="8", RT_REHEARSE_DEVICES="8")
    r = subprocess.run([exe, "1", "1200", "10", "_"], cwd=str(tmp_path), env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    data = open(os.path.join(str(tmp_path), "output.tiff"), "rb").read()
    e = manifest["renders"]["s1_1200x675_10spp_d50"]
    assert hashlib.sha256(data[168:]).hexdigest() == e["sha256"]


@pytest.mark.parametrize("world", [2, 8])
def test_render_share_reassembles_reference_frame(manifest, world, monkeypatch):
    """rt_render_share (one process or thread per GPU, r06): every share of a `world`-way partition,
    written into one host frame, is the reference frame -- from an empty device-scene cache, again from
    the warm cache (no upload: the scene, its record arena and its rows reused), and with the cache off."""
    e = manifest["renders"]["s1_1200x675_10spp_d50"]
    sc = rtc.Scene.preset(1, 1200, 10, 50)
    for cache in ("1", "1", "0"):
        monkeypatch.setenv("RT_SCENE_CACHE", cache)
        out = np.zeros((sc.height, sc.width, 3), np.uint8)
        for g in range(world):
            rtc.render_share(sc, g, world, 0, out)
            ms = rtc.last_share_ms(g)
            assert ms["total"] >= ms["run"] > 0.0
        assert hashlib.sha256(out.tobytes()).hexdigest() == e["sha256"], (world, cache)
    with pytest.raises(rtc.RtcError, match="share"):
        rtc.render_share(sc, world, world, 0)
    rtc.release_cache()


def test_device_scene_cache_follows_scene_and_environment(manifest, monkeypatch):
    """The device-scene cache is keyed by the flat scene's bytes and the RT_* environment: alternating
    scenes, spp and a planner knob between rt_render calls must give each configuration's reference
    frame, never a frame of the previously cached scene; rt_render_cache_release empties it."""
    names = ["s1_300x168_16spp_d50", "s0_400x225_100spp_d50", "s1_300x168_16spp_d50", "s5_200x112_16spp_d50",
             "s1_300x168_16spp_d50"]
    for i, name in enumerate(names):
        e = manifest["renders"][name]
        if i == 2:
            monkeypatch.setenv("RT_CHAIN_BETA", "0.5")  # (another key: a new plan, the same frame)
        img = rtc.render(rtc.Scene.preset(e["scene"], e["width"], e["spp"], e["depth"]))
        _check(img, golden_image(e), f"{name} (call {i})")
        img = rtc.render(rtc.Scene.preset(e["scene"], e["width"], e["spp"], e["depth"]))  # warm
        _check(img, golden_image(e), f"{name} (call {i}, warm)")
        assert rtc.last_share_ms(0)["setup"] < 1000.0
    rtc.release_cache()
    e = manifest["renders"]["s1_300x168_16spp_d50"]
    img = rtc.render(rtc.Scene.preset(e["scene"], e["width"], e["spp"], e["depth"]), n_gpus=1)
    _check(img, golden_image(e), "after rt_render_cache_release")
