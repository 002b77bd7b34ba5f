"""SegTrainer.step with and without dropout at the reference's size (321 x 321, 21 classes, the real widths, f16x3, B images), the
sibling of profiles/seg_train_step.py whose inputs it shares.

  python profiles/seg_train_step_dropout.py steps [B] [drop_prob]
      one JSON line per method: `repeats` = five wall times (ms per step, three steps each, the stream drained) of
      SegTrainer(drop_prob=drop_prob).step.  drop_prob 0 (the default) takes no new keyword: the same file runs on a checkout of
      the commit before dropout, which is how the two are compared.
  rocprofv3 --kernel-trace --stats -d DIR -o drop -- python profiles/seg_train_step_dropout.py trace [B]
      three steps of each method at drop_prob = 0.5, nothing timed by the script; then
  python profiles/seg_train_step_dropout.py summarize DIR [B]
      reads the kernel trace and prints, per method-independent kernel name containing "dropout", the launches, the mean / min /
      max duration and the achieved bandwidth against the algorithmic bytes of the launch: per element 4 bytes read (hi + lo),
      4 written, 4 of tape.

Run each GPU step under its own time limit (timeout -k 10 300 ...)."""
import csv
import glob
import json
import os
import re
import sqlite3
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wsss-analysis_amd")]

MODE = sys.argv[1] if len(sys.argv) > 1 else "steps"
B = int(sys.argv[2]) if len(sys.argv) > 2 and MODE != "summarize" else (int(sys.argv[3]) if len(sys.argv) > 3 and MODE == "summarize" else 8)
DROP = float(sys.argv[3]) if len(sys.argv) > 3 and MODE == "steps" else (0.5 if MODE == "trace" else 0.0)
C, HW = 21, (321, 321)
FC_WIDTH, MAP = 1024, (41, 41)
CRF_CFG = {"g_sxy": 3, "g_compat": 3, "bi_sxy": 80, "bi_srgb": 13, "bi_compat": 10, "iterations": 5}
MEAN = np.array([104.00698793, 116.66876762, 122.67891434], np.float32)


def summarize(directory):
    """the dropout launches of a --kernel-trace run: every launch is one site of one step, B * 41 * 41 * 1024 elements"""
    rows = []  # (kernel name, ns)
    for path in glob.glob(os.path.join(directory, "**", "*_results.db"), recursive=True):  # the rocpd database (profiles/summarize_rocpd.py)
        rows += sqlite3.connect(path).execute(
            "SELECT S.display_name, K.end - K.start FROM rocpd_kernel_dispatch K JOIN rocpd_info_kernel_symbol S "
            "ON S.id = K.kernel_id AND S.guid = K.guid WHERE S.display_name LIKE '%dropout%'").fetchall()
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):  # ... or the CSV form
        with open(path) as fh:
            rows += [(r["Kernel_Name"], int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) for r in csv.DictReader(fh) if "dropout" in r["Kernel_Name"]]
    if not rows:
        raise SystemExit("no dropout launch in a kernel trace under %s" % directory)
    us = np.array([ns / 1e3 for _, ns in rows])
    elems = B * MAP[0] * MAP[1] * FC_WIDTH
    nbytes = 12 * elems
    print(json.dumps({"kernel": sorted(set(re.search(r"\w*dropout\w*", name).group(0) for name, _ in rows)), "launches": len(rows), "B": B, "elements": elems,
                      "bytes": nbytes, "mean_us": round(float(us.mean()), 2), "min_us": round(float(us.min()), 2),
                      "max_us": round(float(us.max()), 2), "median_us": round(float(np.median(us)), 2),
                      "median_gbs": round(nbytes / float(np.median(us)) / 1e3, 1)}), flush=True)


if MODE == "summarize":
    summarize(sys.argv[2])
    raise SystemExit(0)

from tests import deeplab_grad_ref as gref  # noqa: E402
from tests import deeplab_ref as ref  # noqa: E402
from wsscam import _lib, secdsrg  # noqa: E402
from wsscam.secdsrg import DeviceMaps  # noqa: E402

ctx = _lib.Context(0)

for method in ("DSRG", "SEC"):
    weights = gref.full_weights(method, C)
    rng = np.random.default_rng(5)
    x = DeviceMaps.from_host(ctx, ref.net_input(B, HW[0], HW[1], 12))
    tags = np.zeros((B, C), np.float32)
    tags[:, 0] = 1
    for b in range(B):
        tags[b, rng.choice(np.arange(1, C), 3, replace=False)] = 1
    kw = {"drop_prob": DROP, "seed": 2024} if DROP > 0 else {}
    tr = secdsrg.SegTrainer(method, weights, C, ctx=ctx, base_lr=1e-9, **kw)  # (a rate that keeps random weights in half's range)
    h, w = tr.net.map_size(*HW)
    assert (h, w) == MAP
    cues = DeviceMaps.from_host(ctx, ((rng.random((B, h, w, C)) < 0.1) * tags[:, None, None, :]).astype(np.float32))

    def steps(n):
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(n):
            new_cues = tr.step(x, cues, tags, MEAN, CRF_CFG)[1]
            if new_cues is not cues:
                new_cues.free()
        ctx.sync()
        return (time.perf_counter() - t0) / n * 1e3

    steps(2)  # the workspaces
    if MODE == "trace":
        steps(3)
    else:
        repeats = [round(steps(3), 2) for _ in range(5)]
        print(json.dumps({"method": method, "B": B, "drop_prob": DROP, "repeats": repeats, "median_ms": float(np.median(repeats)),
                          "spread_ms": round(max(repeats) - min(repeats), 2)}), flush=True)
    for d in (x, cues):
        d.free()
    tr.close()
