#!/usr/bin/env python3
"""Price of replacing a batch's level table (BatchedEnv.set_levels) at the headline geometry (4096 envs, 64x64, pool running),
and the closed-loop period of step() with and without a table.  Not bench.py.

  python tools/levelset_bench.py [--out FILE]

(1) A stepping loop with one set_levels call every 8 steps, HIP events around each call: the time the call's work takes on
the launch stream -- the wait for the world pool's batches in flight and the copy / emptying kernel.  Tables of 16 and of 65536
levels, uniform and weighted, given as device tensors so that no host hashing is in the figures.  (2) Windows of `steps` steps
between device-wide synchronizes with no table, a uniform and a weighted table of 200 levels, alternated over the rounds: a
table adds one dependent global load (plus the search when weighted) at the head of every generation."""
import argparse
import json
import pathlib
import sys
import time

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from crafter_amd import BatchedEnv, state  # noqa: E402


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--envs', type=int, default=4096)
  ap.add_argument('--calls', type=int, default=40)
  ap.add_argument('--steps', type=int, default=1000)
  ap.add_argument('--warmup', type=int, default=200)
  ap.add_argument('--rounds', type=int, default=3)
  ap.add_argument('--out', default='')
  args = ap.parse_args()
  n = args.envs
  rs = np.random.RandomState(0)
  env = BatchedEnv(n, seed=0)
  acts = [torch.from_numpy(rs.randint(0, 17, n).astype(np.int32)).cuda() for _ in range(64)]

  def table(K):
    return torch.from_numpy(state.seed_lanes([10 ** 6 + i for i in range(K)]).view(np.int64)).cuda()
  tabs = {'K=16': (table(16), None), 'K=65536': (table(65536), None),
          'K=65536 weighted': (table(65536), rs.randint(0, 4, 65536) + 1)}
  env.reset()
  for t in range(args.warmup):
    env.step(acts[t % 64], info=False)
  torch.cuda.synchronize()

  def call_window(lanes, weights):
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.calls)]
    for k, (a, b) in enumerate(pairs):
      for t in range(8):
        env.step(acts[(8 * k + t) % 64], info=False)
      a.record()
      env.set_levels(lanes, weights=weights, key=k)
      b.record()
    torch.cuda.synchronize()
    return [1e3 * a.elapsed_time(b) for a, b in pairs]

  def stats(v):
    return {'median': round(float(np.median(v)), 1), 'mean': round(float(np.mean(v)), 1),
            'p10': round(float(np.percentile(v, 10)), 1), 'p90': round(float(np.percentile(v, 90)), 1)}

  res = {'envs': n, 'calls_per_window': args.calls, 'rounds': args.rounds, 'set_levels_us_per_call': {}, 'step_us': {}}
  for name, (lanes, weights) in tabs.items():
    times = []
    for _ in range(args.rounds):
      times += call_window(lanes, weights)
    res['set_levels_us_per_call'][name] = stats(times)

  def step_window():
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(args.steps):
      env.step(acts[t % 64], info=False)
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0) / args.steps

  loops = {'no table': None, 'uniform 200': (table(200), None), 'weighted 200': (table(200), rs.randint(0, 4, 200) + 1)}
  periods = {k: [] for k in loops}
  for _ in range(args.rounds):
    for name, tab in loops.items():
      env.set_levels(None) if tab is None else env.set_levels(tab[0], weights=tab[1])
      step_window()   # (the table's first episodes: every env regenerates inline once)
      periods[name].append(step_window())
  res['step_us'] = {k: [round(x, 2) for x in v] for k, v in periods.items()}
  env.check_errors()
  res['pool'] = env.pool_status()
  print(json.dumps(res))
  if args.out:
    pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(args.out).write_text(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
  main()
