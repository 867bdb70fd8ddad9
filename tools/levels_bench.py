#!/usr/bin/env python3
"""Price of choosing levels at reset (BatchedEnv.reset(mask, seeds=...)) against the plain reset(mask) of the same build, at the
headline geometry (4096 envs, 64x64, pool running).  Not bench.py.

  python tools/levels_bench.py [--out FILE]

A stepping loop with one reset call every 8 steps, HIP events around each call (the time the call's work takes on the launch
stream: the wait for the world pool's batches in flight, the reseed kernel, the reset kernel with its inline generation); the
plain and the seeded variant alternate in one process, for a mask naming 1/16 of the envs and for all envs.  The seeds are
lanes on the device (BatchedEnv.levels() of another batch), so that no host hashing is in the figures."""
import argparse
import json
import pathlib
import sys

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from crafter_amd import BatchedEnv, state  # noqa: E402


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--envs', type=int, default=4096)
  ap.add_argument('--calls', type=int, default=40)
  ap.add_argument('--warmup', type=int, default=200)
  ap.add_argument('--rounds', type=int, default=3)
  ap.add_argument('--out', default='')
  args = ap.parse_args()
  n = args.envs
  rs = np.random.RandomState(0)
  env = BatchedEnv(n, seed=0)
  acts = [torch.from_numpy(rs.randint(0, 17, n).astype(np.int32)).cuda() for _ in range(64)]
  lanes = torch.from_numpy(state.seed_lanes([10 ** 6 + i for i in range(n)]).view(np.int64)).cuda()
  masks = {'1/16': (torch.arange(n) % 16 == 0).to(torch.uint8).cuda(), 'all': torch.ones(n, dtype=torch.uint8).cuda()}
  env.reset()
  for t in range(args.warmup):
    env.step(acts[t % 64], info=False)
  torch.cuda.synchronize()

  def window(mask, seeded):
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.calls)]
    for k, (a, b) in enumerate(pairs):
      for t in range(8):
        env.step(acts[(8 * k + t) % 64], info=False)
      a.record()
      if seeded:
        env.reset(mask, seeds=lanes)
      else:
        env.reset(mask)
      b.record()
    torch.cuda.synchronize()
    return [1e3 * a.elapsed_time(b) for a, b in pairs]

  res = {'envs': n, 'calls_per_window': args.calls, 'rounds': args.rounds, 'us_per_call': {}}
  for name, mask in masks.items():
    times = {'plain': [], 'seeds': []}
    for _ in range(args.rounds):
      times['plain'] += window(mask, False)
      times['seeds'] += window(mask, True)
    res['us_per_call'][name] = {k: {'median': round(float(np.median(v)), 1), 'mean': round(float(np.mean(v)), 1),
                                    'p10': round(float(np.percentile(v, 10)), 1), 'p90': round(float(np.percentile(v, 90)), 1)}
                                for k, v in times.items()}
  env.check_errors()
  res['pool'] = env.pool_status()['state']
  print(json.dumps(res))
  if args.out:
    pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(args.out).write_text(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
  main()
