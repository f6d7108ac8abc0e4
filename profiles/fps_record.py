"""The record of DESIGN.md row f19 (section 8.11): downsample_point_cloud_farthest_point on uniform float32 clouds in the unit cube, device-resident
torch tensors, at 16,384 points / 1,024 samples (the one-block path), 1M / 4,096 and 16M / 4,096 (the grid path), beside what a user writes
today: the torch loop of one distance pass, torch.minimum, exclusion and argmax per sample, on the same device in the same process. Device
milliseconds between two events around the Python call on the current stream, three warm-ups, the median and range of 15 repeats. The loop and
the library must return the same rows at every shape (the loop's arithmetic is the contract's: separate multiplies and adds in float32,
argmax taking the first of equal maxima). Per shape also the grid path's counters: bucket bound tests and bucket updates per iteration.

A/B of compile-time choices: libraries built from the same sources with other defines (__graft_entry__.build_variant; csrc/fps.h:
PCU_FPS_NO_PRUNE, PCU_FPS_BUCKET, PCU_FPS_CHAIN), each timed by a child process of this script that loads it through PCU_HIP_LIBRARY:
    python profiles/fps_record.py [out.json] [name=path/to/libpcu_hip_variant.so ...]
Writes profiles/fps_record.json (or the path given)."""
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
import point_cloud_utils_amd as pcu
from point_cloud_utils_amd import _fps

SHAPES = [(16_384, 1_024), (1_000_000, 4_096), (16_000_000, 4_096)]
REPS = 15


def device_ms(fn, reps=REPS, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return {"ms_median": round(float(np.median(ts)), 3), "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3)}


def torch_loop(p, m, start=0):
    """What a user holds today. Nothing crosses to the host inside the loop (the argmax stays a tensor)."""
    n = p.shape[0]
    mind = torch.full((n,), float("inf"), dtype=p.dtype, device=p.device)
    idx = torch.empty((m,), dtype=torch.int64, device=p.device)
    cur = torch.tensor(start, device=p.device)
    neg = torch.tensor(-1.0, dtype=p.dtype, device=p.device)
    for t in range(m):
        idx[t] = cur
        d = p - p[cur]
        sq = d * d
        mind = torch.minimum(mind, (sq[:, 0] + sq[:, 1]) + sq[:, 2])
        mind[cur] = neg                                    # excluded for good: min(-1, d2) stays -1
        cur = torch.argmax(mind)
    return idx


def cloud(n):
    return torch.from_numpy(np.random.default_rng(31).random((n, 3), dtype=np.float32)).cuda()


def time_library(shapes, reps):
    out = {}
    for n, m in shapes:
        p = cloud(n)
        out["%d_%d" % (n, m)] = device_ms(lambda: pcu.downsample_point_cloud_farthest_point(p, m), reps=reps)
        print(n, m, out["%d_%d" % (n, m)], flush=True)
        del p
    return out


def child():
    """Timed under another library (PCU_HIP_LIBRARY): the grid-path shapes only, the geometry it was built with."""
    print("CHILD " + json.dumps({"geometry": _fps._geometry(), "times": time_library(SHAPES[1:], 7)}))


def main(path, variants):
    L, B, G, C = _fps._geometry()
    out = {"dtype": "float32", "device": torch.cuda.get_device_name(0), "reps": REPS,
           "geometry": {"one_block_rows": L, "bucket": B, "blocks": G, "iterations_per_replay": C}, "shapes": {}}
    for n, m in SHAPES:
        p = cloud(n)
        r = {"points": n, "samples": m, "path": "one block" if n <= L else "grid"}
        got = pcu.downsample_point_cloud_farthest_point(p, m)
        r["rows_equal_torch_loop"] = bool((got == torch_loop(p, m)).all())
        r["library"] = device_ms(lambda: pcu.downsample_point_cloud_farthest_point(p, m))
        r["torch_loop"] = device_ms(lambda: torch_loop(p, m))
        r["ratio_loop_over_library"] = round(r["torch_loop"]["ms_median"] / r["library"]["ms_median"], 2)
        r["library_us_per_sample"] = round(1e3 * r["library"]["ms_median"] / m, 3)
        if n > L:
            pcu.set_timing(2)
            c = _fps._forced(p, m, path=None)[2]
            st = pcu.last_stats()
            pcu.set_timing(0)
            r["buckets"] = -(-n // B)
            r["bucket_tests_per_iteration"] = round(int(c[0]) / (m - 1), 1)
            r["bucket_updates_per_iteration"] = round(int(c[1]) / (m - 1), 1)
            r["phases_ms"] = {k: round(v, 3) for k, v in st.items() if k.startswith("ms_") and v}
        out["shapes"]["%d_%d" % (n, m)] = r
        print(r, flush=True)
        del p, got
    out["variants"] = {}
    for spec in variants:
        name, lib = spec.split("=", 1)
        env = dict(os.environ, PCU_HIP_LIBRARY=os.path.abspath(lib))
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, timeout=900)
        line = [ln for ln in res.stdout.splitlines() if ln.startswith("CHILD ")]
        out["variants"][name] = json.loads(line[-1][6:]) if line and res.returncode == 0 else {"failed": res.returncode, "stderr": res.stderr[-500:]}
        print(name, out["variants"][name], flush=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    if "--child" in sys.argv:
        child()
    else:
        args = [a for a in sys.argv[1:]]
        paths = [a for a in args if "=" not in a]
        main(paths[0] if paths else os.path.join(os.path.dirname(os.path.abspath(__file__)), "fps_record.json"), [a for a in args if "=" in a])
