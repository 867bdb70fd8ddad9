#!/usr/bin/env python3
"""Writes tests/golden/reference_runs/oracle_vs_reference.npz: the runs of tests/reference_runs.py played on the UNTOUCHED reference
(imported through oracle/reference_harness.py), as digests, for tests/test_oracle_vs_reference.py to replay on the
oracle.  Needs the reference tree (CRAFTER_REFERENCE); like tools/make_golden.py it is run where that tree exists:

    PYTHONDONTWRITEBYTECODE=1 python tools/make_reference_runs.py

Besides the runs: the worlds of the exp-tie tests, once with worldgen's np.exp replaced by the C library's exp (correctly
rounded on the tie cells, tests/test_exp_cr.py) and once as the reference runs on this host, with the flavour of this
host's np.exp recorded beside them (oracle/exp_cr.py explains why the flavour decides a material on rare worlds)."""
import json
import math
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.dont_write_bytecode = True

from oracle import reference_harness as rh  # noqa: E402
from tests import reference_runs as rr  # noqa: E402

TIE_WORLD = (7327, 11)   # seed, episodes: episode 10 holds the tie cell (32, 28)


class _NumpyWithLibmExp:
  """`np` as crafter.worldgen sees it, with exp() = the C library's; everything else is numpy's."""

  def __getattr__(self, name):
    return getattr(np, name)

  @staticmethod
  def exp(x):
    return np.float64(math.exp(float(x)))


def make_reference(**kw):
  env = rh.load().Env(**kw)
  return env, rr.ReferenceSide(env)


def reference_worlds(seed, episodes, libm_exp):
  from crafter import worldgen
  saved = worldgen.np
  if libm_exp:
    worldgen.np = _NumpyWithLibmExp()
  try:
    return rr.worlds(make_reference, seed, episodes)
  finally:
    worldgen.np = saved


def main():
  rh.load()
  out = {}
  for name, run in rr.RUNS.items():
    out[f'run_{name}'] = np.array(run(make_reference), np.uint64)
    print(name, len(out[f'run_{name}']), 'rows')
  libm = reference_worlds(*TIE_WORLD, libm_exp=True)
  host = reference_worlds(*TIE_WORLD, libm_exp=False)
  out['tie_world_libm_exp'] = np.array([(rr.digest(m), o) for m, o in libm], np.uint64)
  out['tie_world_host_exp_mat'] = np.stack([m for m, _ in host]).astype(np.uint8)
  out['tie_world_host_exp_objects'] = np.array([o for _, o in host], np.uint64)
  ties = json.loads((ROOT / 'tests' / 'golden' / 'exp_ties.json').read_text())
  rows = []
  for t in ties['ties'] + ties['decided_differently_by_this_hosts_np_exp']['first']:
    (lm, lo), (hm, ho) = (reference_worlds(t['seed'], t['episode'], libm_exp=f)[-1] for f in (True, False))
    rows.append((rr.digest(lm), lo, rr.digest(hm), ho))
  out['sweep_ties'] = np.array(rows, np.uint64)   # (mat, objects) with libm's exp, then with this host's np.exp
  out['host_np_exp_misrounds'] = np.array(np.exp(np.float64(-1.638387376145862e-16)).hex() != '0x1.fffffffffffffp-1')
  path = ROOT / 'tests' / 'golden' / rr.FIXTURE
  path.parent.mkdir(exist_ok=True)
  np.savez_compressed(path, **out)
  print(path, path.stat().st_size, 'bytes')


if __name__ == '__main__':
  main()
