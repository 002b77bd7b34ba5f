"""DSRG seeded region growing at the reference's size: 41 x 41 x 21 (model.py:35), B = 16 (an assumption: the reference takes
its batch size from the command line), three foreground tags per image, inputs of tests/dsrg_ref.make_case.

Prints one JSON line: kernel time of wsc_dsrg_seed_grow (device events, buffers resident), wall time of
secdsrg.generate_seed_step (upload + call + download), and the vectorised numpy / scipy oracle on the same inputs on the host.
The oracle is NOT the reference's code: that is a per-pixel Python scan plus a Python labeller that is missing from the
reference tree, behind a process pool -- slower than the oracle by a wide margin that cannot be measured here.

One GPU step; run it under its own time limit:   timeout -k 10 120 python profiles/dsrg_grow.py"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wsss-analysis_amd")]
from tests import dsrg_ref  # noqa: E402
from wsscam import _lib, secdsrg  # noqa: E402

B, H, W, C, N_FG, REPS = 16, 41, 41, 21, 3, 200

ctx = _lib.Context(0)
tags, cues, probs = dsrg_ref.make_case(np.random.default_rng(7), B, H, W, C, N_FG)
ref, grown, blocked = dsrg_ref.seed_grow_batch(tags, cues, probs)

t_dev, c_dev, p_dev = (ctx.to_device(a) for a in (tags, cues, probs))
o_dev = ctx.alloc(cues.nbytes)
call = lambda: _lib.dsrg_seed_grow(ctx, t_dev, c_dev, p_dev, B, H, W, C, o_dev)  # out of place: every repeat does the same work
for _ in range(10):
    call()
assert np.array_equal(ctx.to_host(o_dev, cues.shape, np.float32), ref)
ctx.timer_begin()
for _ in range(REPS):
    call()
kernel_ms = ctx.timer_end() / REPS

step = lambda: secdsrg.generate_seed_step(tags, cues, probs, ctx=ctx)
for _ in range(10):
    assert np.array_equal(step(), ref)
t0 = time.perf_counter()
for _ in range(REPS):
    step()
wall_ms = (time.perf_counter() - t0) / REPS * 1e3

t0 = time.perf_counter()
for _ in range(5):
    dsrg_ref.seed_grow_batch(tags, cues, probs)
oracle_ms = (time.perf_counter() - t0) / 5 * 1e3

print(json.dumps({"shape": [B, H, W, C], "fg_tags": N_FG, "grown": grown, "blocked": blocked, "reps": REPS,
                  "kernel_ms_per_batch": round(kernel_ms, 4), "wall_ms_per_batch": round(wall_ms, 4),
                  "numpy_oracle_ms_per_batch": round(oracle_ms, 3)}))
