#!/usr/bin/env python3
"""Where should the Huffman decode of a JPEG run? ``decode_jpeg(entropy="device")`` against ``decode_jpeg(entropy="host")`` (the
path of every earlier commit, unchanged) in one build on one card, alternated, on the COCO fixture as stored, a 900 x 1600 and a
1080 x 1920 quality-90 4:2:0 picture. Per input and route, warm, the median of N (default 30):

- wall time of ``decode_jpeg`` up to the finished picture (a device synchronise closes the window);
- the call's host CPU time (``time.thread_time`` around the same window): what the device route is for, since a GPU machine gives a
  job 16 CPUs for 8 cards;
- device time by HIP events around the stream work alone (upload, kernels), buffers allocated before;
- bytes uploaded, relaxation rounds.

The host leg is cross-checked against profiles/r02/bench_r02_jpeg.jsonl. Writes README.md and bench_jpeg_decode.json into the
directory given (default profiles/jpeg_decode) and prints one JSON line: ``python tools/bench_jpeg_decode.py [OUTDIR] [N]``."""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import jpeg_entropy_cases as K  # noqa: E402
from test_jpeg import COCO, _jpeg, _pil, _scene  # noqa: E402
from ovmono3d_amd import lib as _lib  # noqa: E402
from ovmono3d_amd.data import gpu_jpeg  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "jpeg_decode")
N = int(sys.argv[2]) if len(sys.argv) > 2 else 30
WARM = 5
if not torch.cuda.is_available():
    raise SystemExit("bench_jpeg_decode.py measures on the HIP device; none found")
dev = torch.device("cuda", 0)
L = _lib.load()


def inputs():
    yield "coco_480x640_as_stored", open(COCO, "rb").read()
    yield "scene_900x1600_q90_420", _jpeg(_scene(900, 1600, 9), quality=90, subsampling=2)
    yield "scene_1080x1920_q90_420", _jpeg(_scene(1080, 1920, 9), quality=90, subsampling=2)


def verdict(dev_ms, host_ms):
    """Does the device route win? A difference under 5 % is inside what two runs of the same route differ by: "level"."""
    if abs(dev_ms - host_ms) <= 0.05 * host_ms:
        return "level"
    return "yes" if dev_ms < host_ms else "no"


def med(ts):
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}


def call_times(data, route):
    """Wall and host CPU time of decode_jpeg, in ms."""
    for _ in range(WARM):
        gpu_jpeg.decode_jpeg(data, dev, entropy=route)
    torch.cuda.synchronize()
    wall, cpu = [], []
    for _ in range(N):
        torch.cuda.synchronize()
        c0, t0 = time.thread_time(), time.perf_counter()
        gpu_jpeg.decode_jpeg(data, dev, entropy=route)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        cpu.append((time.thread_time() - c0) * 1e3)
    return med(wall), med(cpu)


def enqueue_cpu_time(data):
    """Host CPU time of the device route up to the point where the status is waited for (plan, pinned copy, allocations, the call):
    the CPU work proper; what follows in decode_jpeg is a wait that other work could fill. ms."""
    for _ in range(WARM):
        gpu_jpeg._entropy_enqueue(data, dev)
    torch.cuda.synchronize()
    ts = []
    for _ in range(N):
        torch.cuda.synchronize()
        c0 = time.thread_time()
        keep = gpu_jpeg._entropy_enqueue(data, dev)
        ts.append((time.thread_time() - c0) * 1e3)
        torch.cuda.synchronize()
        del keep
    return med(ts)


def device_times(data):
    """HIP events around the stream work of each route (upload + kernels), everything allocated before: ms."""
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    coef_h, info = gpu_jpeg.entropy_decode(data, pin=True)
    nb = int(info.coef_blocks)
    planes = torch.empty(nb * 64, dtype=torch.uint8, device=dev)
    rgb = torch.empty((int(info.height), int(info.width), 3), dtype=torch.uint8, device=dev)
    coef_d = torch.empty((nb, 64), dtype=torch.int16, device=dev)
    plan, tables = gpu_jpeg._decode_plan(data, None)
    n = int(plan.ecs_bytes)
    tb = tables.size
    host = torch.empty(tb + n, dtype=torch.uint8, pin_memory=True)
    host.numpy()[:tb] = tables
    host.numpy()[tb:] = np.frombuffer(data, dtype=np.uint8, count=n, offset=int(plan.ecs_offset))
    blob = torch.empty(tb + n, dtype=torch.uint8, device=dev)
    wsb = C.c_int64()
    _lib.check(L.ovm_jpeg_entropy_decode_workspace(C.byref(plan), C.byref(wsb)))
    ws = torch.empty(int(wsb.value), dtype=torch.uint8, device=dev)
    result = torch.zeros(3, dtype=torch.int32, device=dev)

    def host_route():
        coef_d.copy_(coef_h, non_blocking=True)
        _lib.check(L.ovm_jpeg_reconstruct(coef_d.data_ptr(), C.byref(info), planes.data_ptr(), rgb.data_ptr(), stream))

    def device_route():
        blob.copy_(host, non_blocking=True)
        _lib.check(L.ovm_jpeg_entropy_decode(blob.data_ptr() + tb, blob.data_ptr(), C.byref(plan), ws.data_ptr(), ws.numel(), coef_d.data_ptr(),
                                             coef_d.numel(), result.data_ptr(), stream))
        _lib.check(L.ovm_jpeg_reconstruct(coef_d.data_ptr(), C.byref(info), planes.data_ptr(), rgb.data_ptr(), stream))

    def entropy_only():
        _lib.check(L.ovm_jpeg_entropy_decode(blob.data_ptr() + tb, blob.data_ptr(), C.byref(plan), ws.data_ptr(), ws.numel(), coef_d.data_ptr(),
                                             coef_d.numel(), result.data_ptr(), stream))

    res = {}
    for name, fn in (("host_route_upload_and_reconstruct", host_route), ("device_route_upload_entropy_reconstruct", device_route),
                     ("ovm_jpeg_entropy_decode_alone", entropy_only)):
        for _ in range(WARM):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(N):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        res[name] = med(ts)
    status, rounds, launches = result.tolist()
    res.update(status=status, rounds=rounds, productive_launches=launches, workspace_bytes=int(wsb.value), upload_bytes_device_route=tb + n, upload_bytes_host_route=nb * 128,
               subsequences=-(-K.unstuffed_len(data, plan) * 8 // plan.sub_bits), sub_bits=int(plan.sub_bits), wg_subs=int(plan.wg_subs),
               sync_launches=int(plan.sync_launches), max_rounds=int(plan.max_rounds))
    return res


r02 = {}
with open(os.path.join(ROOT, "profiles", "r02", "bench_r02_jpeg.jsonl")) as f:
    for line in f:
        if line.strip():
            row = json.loads(line)
            r02[row["case"]] = row
R02_OF = {"coco_480x640_as_stored": "coco_480x640_420", "scene_1080x1920_q90_420": "1080p_420"}

props = torch.cuda.get_device_properties(0)
res = {"device": torch.cuda.get_device_name(0), "arch": str(getattr(props, "gcnArchName", "")), "compute_units": int(props.multi_processor_count),
       "n": N, "warmup": WARM, "inputs": {}}
for name, data in inputs():
    r = {"file_bytes": len(data)}
    ref = _pil(data)
    for route in ("host", "device"):
        r[f"equal_to_pillow_{route}"] = bool(np.array_equal(gpu_jpeg.decode_jpeg(data, dev, entropy=route).cpu().numpy(), ref))
    r.update(device_times(data))
    r["device_cpu_before_status_wait_ms"] = enqueue_cpu_time(data)
    # the two routes alternate, twice, so that whatever else the host is doing falls on both
    rounds_of = {"host": [], "device": []}
    for _ in range(2):
        for route in ("host", "device"):
            rounds_of[route].append(call_times(data, route))
    for route in ("host", "device"):
        best = min(rounds_of[route], key=lambda wc: wc[0]["median"])
        r[f"{route}_wall_ms"], r[f"{route}_cpu_ms"] = best
        r[f"{route}_wall_ms_both_rounds"] = [wc[0]["median"] for wc in rounds_of[route]]
    r["device_route_wins_wall"] = verdict(r["device_wall_ms"]["median"], r["host_wall_ms"]["median"])          # "yes" / "level" / "no"
    r["device_route_wins_host_cpu"] = verdict(r["device_cpu_ms"]["median"], r["host_cpu_ms"]["median"])
    if name in R02_OF:
        r["r02_split_decode_end_to_end_ms"] = r02[R02_OF[name]]["split_decode_end_to_end_ms"]
        r["r02_file_bytes"] = r02[R02_OF[name]]["jpeg_bytes"]
    res["inputs"][name] = r

# files that synchronise slowly: all components on one table pair (the COCO fixture re-saved as RGB without a colour transform), where the
# tables say nothing about the block index, and quality-100 noise, where almost every bit string is a valid code
def slow_files():
    import io
    from PIL import Image
    with Image.open(COCO) as im:
        b = io.BytesIO()
        im.convert("RGB").save(b, format="JPEG", quality=90, keep_rgb=True)
    yield "coco_rgb_one_table_pair_q90", b.getvalue()
    yield "noise_300x400_q100_420", _jpeg(np.random.default_rng(1).integers(0, 256, (300, 400, 3), dtype=np.uint8), quality=100, subsampling=2)


res["slow_to_synchronise"] = {}
for name, data in slow_files():
    d = {"file_bytes": len(data)}
    d["equal_to_pillow_device"] = bool(np.array_equal(gpu_jpeg.decode_jpeg(data, dev, entropy="device").cpu().numpy(), _pil(data)))
    d.update(device_times(data))
    (d["host_wall_ms"], _), (d["device_wall_ms"], _) = call_times(data, "host"), call_times(data, "device")
    res["slow_to_synchronise"][name] = d

# round counts of the test files, from the CPU emulation (tests/test_gpu_jpeg_entropy.py asserts the kernels use the same number)
res["test_file_rounds"] = {n: {"subsequences": -(-K.unstuffed_len(K.well_formed()[n], K.plan_of(K.well_formed()[n])[1]) * 8 // 512),
                               "rounds": K.emulated(n)[3], "productive_launches": K.emulated_launches(n)} for n in sorted(K.well_formed())}

os.makedirs(OUT, exist_ok=True)
with open(os.path.join(OUT, "bench_jpeg_decode.json"), "w") as f:
    json.dump(res, f, indent=1)

any_in = next(iter(res["inputs"].values()))
lines = ["# JPEG Huffman decode on the device (`ovm_jpeg_entropy_decode`, `decode_jpeg(entropy=\"device\")`)", "",
         "Written by `python tools/bench_jpeg_decode.py` (raw numbers: `bench_jpeg_decode.json`) on one " + res["device"] + " (" + res["arch"] + ", " +
         str(res["compute_units"]) + " compute units: an Instinct MI355X).",
         f"Both routes in one build, alternated twice; {WARM} warm-up calls, then the median of {N}; the better of the two medians per route",
         "is shown (both are in the JSON). `entropy=\"host\"` is the path of every earlier commit, unchanged. In every row both routes",
         "return Pillow's pixels (`equal_to_pillow_*` in the JSON).", "",
         "| input | file | wall, host route | wall, device route | host CPU, host route | host CPU, device route | of which before the status wait | uploaded, host / device route | rounds |",
         "|---|---|---|---|---|---|---|---|---|"]
for name, r in res["inputs"].items():
    lines.append(f"| {name} | {r['file_bytes']:,} B | {r['host_wall_ms']['median']:.3f} ms | {r['device_wall_ms']['median']:.3f} ms | "
                 f"{r['host_cpu_ms']['median']:.3f} ms | {r['device_cpu_ms']['median']:.3f} ms | {r['device_cpu_before_status_wait_ms']['median']:.3f} ms | "
                 f"{r['upload_bytes_host_route']:,} / {r['upload_bytes_device_route']:,} B | {r['rounds']} |")
lines += ["", "Device time (HIP events around the stream work alone, buffers allocated and pinned before):", "",
          "| input | host route: coefficient upload + reconstruct | device route: file upload + entropy decode + reconstruct | `ovm_jpeg_entropy_decode` alone |",
          "|---|---|---|---|"]
for name, r in res["inputs"].items():
    lines.append(f"| {name} | {r['host_route_upload_and_reconstruct']['median']:.3f} ms | {r['device_route_upload_entropy_reconstruct']['median']:.3f} ms | "
                 f"{r['ovm_jpeg_entropy_decode_alone']['median']:.3f} ms |")
lines += ["", "**Does the device route win?**", ""]
for name, r in res["inputs"].items():
    lines.append(f"- {name}: wall time {r['device_route_wins_wall']} "
                 f"({r['device_wall_ms']['median']:.3f} against {r['host_wall_ms']['median']:.3f} ms); host CPU time of the call "
                 f"{r['device_route_wins_host_cpu']} "
                 f"({r['device_cpu_ms']['median']:.3f} against {r['host_cpu_ms']['median']:.3f} ms; "
                 f"{r['device_cpu_before_status_wait_ms']['median']:.3f} ms of it before the status wait).")
lines += ["", "(\"level\": within 5 %, which is what two runs of the same route differ by.)"]
lines += ["", "The host CPU time of the device route is almost all wait: `decode_jpeg` reads the status word back before it chooses the",
          "route, and the runtime spins while it waits, so the thread's CPU time follows the device time. The column \"before the status",
          "wait\" is the CPU work proper - plan (header walk, one `memchr` pass over the scan), the copy of the file's bytes into pinned",
          "memory, allocations, the call; a loader that decodes several images would fill the wait with the next image's plan, which",
          "`decode_jpeg` as it stands does not do.", "",
          "Cross-check of the host leg against `profiles/r02/bench_r02_jpeg.jsonl` (`split_decode_end_to_end_ms`, measured then on the same kind of card):", ""]
for name, r in res["inputs"].items():
    if "r02_split_decode_end_to_end_ms" in r:
        lines.append(f"- {name}: {r['host_wall_ms']['median']:.3f} ms now, {r['r02_split_decode_end_to_end_ms']:.3f} ms then "
                     f"(file {r['file_bytes']:,} B now, {r['r02_file_bytes']:,} B then).")
lines += ["", "## Subsequence size, round cap, round counts", "",
          f"Subsequences of {any_in['sub_bits']} bits, {any_in['wg_subs']} per workgroup, {any_in['sync_launches']} synchronisation launches per call; default",
          f"`max_rounds` {any_in['max_rounds']} relaxation steps per workgroup and launch (the workgroup's subsequence count, at which it is certainly",
          "consistent). `rounds` is the sum over the launches of the largest step count of any workgroup. Counts of the test files",
          "(CPU emulation; the GPU tests assert that the kernels report the same). A file is turned over to the host when a workgroup",
          f"needs more than the cap in one launch or when more than {any_in['sync_launches'] - 1} launches decode anything (a clean launch must follow the last productive",
          "one); the last column is what each file used of those:", "", "| file | subsequences | rounds | productive launches |", "|---|---|---|---|"]
for n, v in res["test_file_rounds"].items():
    lines.append(f"| {n} | {v['subsequences']} | {v['rounds']} | {v['productive_launches']} |")
for name, r in res["inputs"].items():
    lines.append(f"| {name} (bench input, device) | {r['subsequences']} | {r['rounds']} | {r['productive_launches']} |")
big = max(v["rounds"] for v in res["test_file_rounds"].values())
lines += ["", f"Largest count among the test files: {big}; the default cap is {any_in['max_rounds'] / big:.1f} times that. Most productive launches: "
          f"{max(v['productive_launches'] for v in res['test_file_rounds'].values())} of {any_in['sync_launches'] - 1}.", "",
          "## Files that synchronise slowly, and what a declined file costs", "",
          "| file | size | subsequences | status | rounds | productive launches | `ovm_jpeg_entropy_decode` | `decode_jpeg` device / host route |",
          "|---|---|---|---|---|---|---|---|"]
for name, d in res["slow_to_synchronise"].items():
    lines.append(f"| {name} | {d['file_bytes']:,} B | {d['subsequences']} | {d['status']} | {d['rounds']} | {d['productive_launches']} | "
                 f"{d['ovm_jpeg_entropy_decode_alone']['median']:.2f} ms | {d['device_wall_ms']['median']:.2f} / {d['host_wall_ms']['median']:.2f} ms |")
lines += ["", "The device time follows the rounds (about 40 us each). A stream that never falls in step is declined only after every launch has run",
          f"its {any_in['max_rounds']} steps, {any_in['sync_launches']} x {any_in['max_rounds']} rounds: with the block index taken modulo the MCU's block count instead of the",
          "period of its table pairs, the one-table-pair file above did exactly that - status 4 after 1,536 rounds, 69.97 ms of device time, then",
          "the host decoder (71.87 ms for `decode_jpeg` against 1.80 ms on the host route). That is what the cap admits for a hostile file of that",
          "size; `max_rounds` lowers it.", ""]
with open(os.path.join(OUT, "README.md"), "w") as f:
    f.write("\n".join(lines))
print(json.dumps(res))
