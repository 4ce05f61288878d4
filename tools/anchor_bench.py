#!/usr/bin/env python3
"""Autoanchor wall time: the device's k-means and evolution (anchors.py; yf_anchor_kmeans, yf_anchor_evolve) against the transcription of
yolov5's evolve loop in torch on the CPU (tests/anchor_v5_ref.py) and, where scipy is installed, scipy's k-means as yolov5 calls it.
GPU box:
    python tools/anchor_bench.py       synthetic label shapes (three log-normal clusters, seed 1) at 10^4, 10^5 and 10^6 labels, 6 anchors,
                                       thr 4, 30 restarts, 1000 generations from np.random.seed(0) / random.seed(0).  Per size: the
                                       device k-means (passes = its longest restart + 1 for the fit), the device evolution from the
                                       k-means' anchors (passes over the labels, accepted generations), the transcription's evolution
                                       from the same anchors and draws (--cpu-gen-large generations at 10^6, the time scaled to 1000 and
                                       marked so), whether the two chains accepted the same generations up to there, scipy's
                                       kmeans(wh / s, 6, iter=30); then one JSON line.  One run each, after one untimed device call:
                                       a record, not a statistic.  The float32 mean of the transcription and the exact sum of the rule
                                       can part where a decision lies within that rounding; the line says whether they did."""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import anchor_v5_ref  # noqa: E402
from yolo_fastest_amd import anchors as aa  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", type=int, nargs="+", default=[10 ** 4, 10 ** 5, 10 ** 6])
ap.add_argument("--gen", type=int, default=1000)
ap.add_argument("--cpu-gen-large", type=int, default=100, help="generations the transcription runs at 10^6 labels and above")
ap.add_argument("--restarts", type=int, default=30)
ap.add_argument("--no-scipy", action="store_true")
a = ap.parse_args()
dev = torch.device("cuda:0")
BASES = np.array([[20, 12], [60, 40], [150, 110]], float)


def labels(n):
    rs = np.random.RandomState(1)
    wh0 = BASES[rs.randint(0, 3, n)] * np.exp(rs.randn(n, 2) * 0.35)
    return wh0[(wh0 >= 2.0).any(1)].astype(np.float32)


def timed(fn):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return out, time.perf_counter() - t0


def main():
    try:
        from scipy.cluster.vq import kmeans as scipy_kmeans
    except ImportError:
        scipy_kmeans = None
    aa.anchor_metric(labels(1000), [[10, 10]], 4.0, dev)                  # untimed: loads the library, creates the context
    rows = []
    for n in a.sizes:
        wh = labels(n)
        np.random.seed(0)
        random.seed(0)
        init = np.stack([np.random.choice(len(wh), 6, replace=False) for _ in range(a.restarts)])
        v = aa.draw_mutations(a.gen, (6, 2))
        (k, winner, iters), t_km = timed(lambda: aa.device_kmeans(wh, 6, init, 4.0, device=dev))
        k = k[np.argsort(k.prod(1))]
        (kd, fit, acc), t_ev = timed(lambda: aa.device_evolve(wh, k, v, 4.0, dev))
        cpu_gen = a.gen if n < 10 ** 6 else min(a.gen, a.cpu_gen_large)
        t0 = time.perf_counter()
        _, vacc, _ = anchor_v5_ref.evolve(wh, k, 4.0, cpu_gen, v=v)
        t_cpu = (time.perf_counter() - t0) * a.gen / cpu_gen
        same = vacc == [int(g) for g in np.flatnonzero(acc) if g < cpu_gen]
        row = {"labels": len(wh), "kmeans_s": t_km, "kmeans_passes": int(iters.max()) + 1, "kmeans_winner": winner,
               "kmeans_discarded": int((iters < 0).sum()), "evolve_s": t_ev, "evolve_passes": aa.evolve_passes(acc), "accepted": int(acc.sum()),
               "v5_evolve_s": t_cpu, "v5_generations_run": cpu_gen, "same_chain": bool(same), "threads": torch.get_num_threads()}
        if scipy_kmeans is not None and not a.no_scipy:
            t0 = time.perf_counter()
            s = wh.std(0)
            scipy_kmeans(wh / s, 6, iter=30)
            row["scipy_kmeans_s"] = time.perf_counter() - t0
        rows.append(row)
        print("%8d labels: device k-means %.4f s (%d passes, %d of %d restarts discarded), device evolve %.4f s (%d passes, %d accepted); "
              "yolov5's evolve on the CPU %.2f s%s (%d threads), same chain: %s%s"
              % (len(wh), t_km, row["kmeans_passes"], row["kmeans_discarded"], a.restarts, t_ev, row["evolve_passes"], row["accepted"], t_cpu,
                 "" if cpu_gen == a.gen else " (scaled from %d generations)" % cpu_gen, row["threads"], same,
                 "; scipy's k-means %.2f s" % row["scipy_kmeans_s"] if "scipy_kmeans_s" in row else ""), flush=True)
    print(json.dumps({"anchor_bench": rows}))


if __name__ == "__main__":
    main()
