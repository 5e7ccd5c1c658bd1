#!/usr/bin/env python3
"""Time of one KeyFrameDatabase place-recognition query (steps 1 and 2 of DetectNBestCandidates) on the GPU and
through a single-threaded CPU restatement of the reference, at 500, 5 000 and 50 000 KeyFrames (GPU).

Databases: BowVectors of about 1 000 words out of 32 ** 4 (ORBvoc has about 10 ** 6), a trajectory over places
of 25 KeyFrames each; a KeyFrame takes 70 % of its words from its place's pool of 1 300 and the rest at random.
The query is one more view of a place.  Per size:
  * device: HIP events around the three kernels of osg_kfdb_query (median of ``--reps`` calls, each with a
    fresh query id: a repeated id lists nothing), and the wall time of the whole call (upload, kernels, both
    read-backs, synchronised) around KeyFrameDatabase.query;
  * cpu: tests/adapter/kfdb_driver.cpp's ``baseline`` (an inverted file of std::list per word, std::map
    BowVectors merged with lower_bound, one thread: the reference's own data structures), compiled here with
    -O3 -march=native; the whole DetectNBestCandidates, median of the same number of calls.
Both return the same candidates, which is asserted.  Recorded, not gated; a speed-up is whatever the file shows.

    python tools/kfdb_bench.py [--out profiles/kfdb_latency.json] [--sizes 500,5000,50000] [--reps 100]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from orb_slam3_comments_ghr_amd import Context  # noqa: E402
from orb_slam3_comments_ghr_amd import keyframedb as K  # noqa: E402
from orb_slam3_comments_ghr_amd.vocabulary import ORBVocabulary  # noqa: E402
from tools.adapter_arrays import read_arrays, write_arrays  # noqa: E402

N_VOCAB = 32 ** 4
WORDS, POOL, PER_PLACE, OWN = 1000, 1300, 25, 0.7


def view(rng, pool):
    own = rng.choice(pool, int(WORDS * OWN), replace=False)
    w = np.unique(np.concatenate([own, rng.integers(0, N_VOCAB, WORDS - len(own))])).astype(np.int32)
    v = rng.uniform(0.2, 1.0, len(w))
    return w, v / v.sum()


def build(n, seed):
    rng = np.random.default_rng(seed)
    n_places = max(n // PER_PLACE, 1)
    pools = [rng.choice(N_VOCAB, POOL, replace=False) for _ in range(n_places)]
    place = np.arange(n) % n_places          # the trajectory passes every place PER_PLACE times
    kfs = [view(rng, pools[place[i]]) for i in range(n)]
    query = view(rng, pools[n_places // 2])
    neigh = [[j for j in range(i - 5, i + 6) if j != i and 0 <= j < n] for i in range(n)]
    return kfs, query, neigh


def csr(lists, dtype):
    start = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int32)
    return start, (np.concatenate(lists).astype(dtype) if lists else np.zeros(0, dtype))


def cpu_baseline(exe, tmp, kfs, query, neigh, reps):
    n = len(kfs)
    a = {"kf.id": np.arange(n, dtype=np.int32), "kf.map": np.zeros(n, np.int32), "kf.bad": np.zeros(n, np.uint8),
         "map.bad": np.zeros(1, np.uint8), "reps": np.array([reps], np.int32), "n_words": np.array([N_VOCAB], np.int32),
         "q.id": np.array([1], np.int32), "q.map": np.zeros(1, np.int32), "q.conn_start": np.zeros(2, np.int32),
         "q.conn": np.zeros(0, np.int32)}
    a["kf.bow_start"], a["kf.word"] = csr([w for w, _ in kfs], np.int32)
    a["kf.value"] = csr([v for _, v in kfs], np.float64)[1]
    a["kf.neigh_start"], a["kf.neigh"] = csr([np.array(l, np.int32) for l in neigh], np.int32)
    a["q.bow_start"], a["q.word"] = csr([query[0]], np.int32)
    a["q.value"] = query[1]
    fi, fo = os.path.join(tmp, "in"), os.path.join(tmp, "out")
    write_arrays(fi, a)
    subprocess.run([exe, "baseline", fi, fo], check=True, timeout=900)
    out = read_arrays(fo)
    os.remove(fi)
    return [float(x) for x in out["ms"]], [int(x) for x in out["cand"]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kfdb_latency.json"))
    ap.add_argument("--sizes", default="500,5000,50000")
    ap.add_argument("--reps", type=int, default=100)
    a = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix="kfdb_bench")
    exe = os.path.join(tmp, "kfdb_driver")
    pkg = os.path.join(ROOT, "orb_slam3_comments_ghr_amd")
    subprocess.run(["g++", "-std=c++17", "-O3", "-march=native", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "adapter", "kfdb_driver.cpp"), "-o", exe, "-L" + pkg, "-lorbslam3_amd",
                    "-Wl,-rpath," + pkg], check=True)
    ctx = Context(0)
    voc = ORBVocabulary(ctx, K.complete_vocabulary(32, 4))
    res = {"device": "MI355X (gfx950)", "vocabulary_words": N_VOCAB, "words_per_keyframe": WORDS, "reps": a.reps,
           "cpu": "kfdb_driver baseline, g++ -O3 -march=native, one thread", "sizes": {}}
    for n in (int(x) for x in a.sizes.split(",")):
        kfs, query, neigh = build(n, 100 + n)
        db = K.KeyFrameDatabase(ctx, voc)
        t0 = time.perf_counter()
        for i, (w, v) in enumerate(kfs):
            db.add(i, (w, v), 0)
        add_ms = 1e3 * (time.perf_counter() - t0) / n
        nb = {i: l for i, l in enumerate(neigh)}
        for r in range(3):                                   # warm-up: code objects, scratch, pinned block
            db.query(K.PLACE, query, 10 + r)
        wall, dev = [], []
        for r in range(a.reps):
            t0 = time.perf_counter()
            q = db.query(K.PLACE, query, 1000 + r)
            wall.append(1e3 * (time.perf_counter() - t0))
            dev.append(ctx.last_kernel_ms())
        loop, merge = db.detect_n_best_candidates(query, 100000 + a.reps - 1, 0, (), nb, 3)
        db.close()
        cpu_ms, cpu_cand = cpu_baseline(exe, tmp, kfs, query, neigh, a.reps)
        assert cpu_cand == loop + merge, (cpu_cand, loop, merge)
        row = {"keyframes": n, "query_words": int(len(query[0])), "n_sharing": q.n_sharing,
               "max_common_words": q.max_common_words, "n_scored": q.n_scored, "candidates": loop + merge,
               "gpu_kernels_ms_median": float(np.median(dev)), "gpu_kernels_ms_min": float(np.min(dev)),
               "gpu_call_wall_ms_median": float(np.median(wall)), "gpu_call_wall_ms_min": float(np.min(wall)),
               "gpu_add_wall_ms_mean": add_ms,
               "cpu_detect_ms_median": float(np.median(cpu_ms)), "cpu_detect_ms_min": float(np.min(cpu_ms))}
        row["cpu_over_gpu_call"] = row["cpu_detect_ms_median"] / row["gpu_call_wall_ms_median"]
        res["sizes"]["kf%d" % n] = row
        print(json.dumps(row), flush=True)
    voc.close()
    ctx.close()
    slower = [r["keyframes"] for r in res["sizes"].values() if r["cpu_over_gpu_call"] < 1.0]
    faster = [r["keyframes"] for r in res["sizes"].values() if r["cpu_over_gpu_call"] >= 1.0]
    res["crossover"] = ("the CPU restatement is faster than the GPU call up to %d KeyFrames and slower from %d" %
                        (max(slower), min(faster)) if slower and faster else
                        "the GPU call is faster at every size measured" if faster else
                        "the CPU restatement is faster at every size measured")
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
