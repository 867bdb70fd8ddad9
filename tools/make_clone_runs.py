#!/usr/bin/env python3
"""Writes tests/golden/reference_runs/deepcopy.npz: what copy.deepcopy and pickle of the UNTOUCHED reference crafter.Env
(imported through oracle/reference_harness.py) do, as digests, for tests/test_clone_host.py to replay on the oracle.  Needs
the reference tree (CRAFTER_REFERENCE); like tools/make_reference_runs.py it is run where that tree exists:

    PYTHONDONTWRITEBYTECODE=1 python tools/make_clone_runs.py

Each case: reset, tape A for k steps, then a copy; the original goes on with tape A, the copy with tape B (a different
tape), both with a reset after every episode end, and a render((512, 512)) at RENDER_AT steps after the branch.  One row
per step (tests/reference_runs.py step_row: obs, reward / done / info, semantic view, objects / chunk order / RNG key and
position), per reset (reset_row) and per render.  The pickle case replays the copy's tape on a pickle round trip."""
import copy
import pathlib
import pickle
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.dont_write_bytecode = True

from tests import reference_runs as rr  # noqa: E402

OUT = ROOT / 'tests' / 'golden' / 'reference_runs' / 'deepcopy.npz'
# (name, seed, length, k = branch step, steps after the branch): length 60 crosses an episode end on both branches; the
# branch at step 160 of a long episode is at night
CASES = [('day_s3', 3, 60, 30, 70), ('day_s11', 11, 60, 30, 70), ('night_s7', 7, 10000, 160, 40)]
RENDER_AT = 15


def tapes(seed, k, steps):
  rs = np.random.RandomState(seed + 1000)
  return rs.randint(0, 17, size=k + steps), rs.randint(0, 17, size=steps)


def branch(env, side, tape, render_at=RENDER_AT):
  rows = []
  for t, a in enumerate(tape):
    result = env.step(int(a))
    rows.append(rr.step_row(side, result))
    if t == render_at:
      rows.append((2, rr.digest(np.asarray(env.render((512, 512)))), 0, 0, 0))
    if result[2]:
      rows.append(rr.reset_row(side, env.reset()))
  return np.array(rows, np.uint64)


def run(make, copier, seed, length, k, steps):
  """make(seed, length) -> (env, side_of(env)).  -> (original's rows, copy's rows) after the branch."""
  env, side_of = make(seed, length)
  a, b = tapes(seed, k, steps)
  env.reset()
  for t in range(k):
    if env.step(int(a[t]))[2]:
      env.reset()
  twin = copier(env)
  return branch(env, side_of(env), a[k:]), branch(twin, side_of(twin), b)


def make_reference(seed, length):
  from oracle import reference_harness as rh
  return rh.load().Env(seed=seed, length=length), rr.ReferenceSide


def pickle_copy(env):
  return pickle.loads(pickle.dumps(env))


def main():
  out = {}
  for name, seed, length, k, steps in CASES:
    orig, twin = run(make_reference, copy.deepcopy, seed, length, k, steps)
    out[f'{name}/meta'] = np.array([seed, length, k, steps], np.int64)
    out[f'{name}/original'] = orig
    out[f'{name}/copy'] = twin
    if name == 'day_s3':
      out[f'{name}/pickle'] = run(make_reference, pickle_copy, seed, length, k, steps)[1]
  OUT.parent.mkdir(parents=True, exist_ok=True)
  np.savez_compressed(OUT, **out)
  print(OUT, OUT.stat().st_size, 'bytes')


if __name__ == '__main__':
  main()
