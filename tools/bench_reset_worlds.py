#!/usr/bin/env python3
"""Price of a reset into authored worlds (BatchedEnv.reset(mask, worlds=bank)) against the plain reset(mask) of the same build,
on the same handle, at the headline geometry (4096 envs, 64x64).  Not bench.py.

  python tools/bench_reset_worlds.py [--out FILE]

A stepping loop with one reset call every 8 steps, HIP events around each call (the time the call's work takes on the launch
stream: the wait for the world pool's batches in flight, the reset kernel and, with the pool on, the next world it generates
into the env's pool entry -- the same tail for both).  The plain and the authored variant alternate in one process, for a mask
naming all envs and for one naming 1 % of them, with the world pool on (auto_reset) and off (where the figure is the kernel's
own work: the authored reset against reset + worldgen).  The bank holds 16 worlds exported from generated ones, so an authored
reset adds as many objects as a generated one places."""
import argparse
import json
import pathlib
import sys

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from crafter_amd import BatchedEnv, WorldBank  # noqa: E402


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--envs', type=int, default=4096)
  ap.add_argument('--calls', type=int, default=30)
  ap.add_argument('--warmup', type=int, default=100)
  ap.add_argument('--rounds', type=int, default=3)
  ap.add_argument('--out', default='')
  args = ap.parse_args()
  n = args.envs
  rs = np.random.RandomState(0)
  res = {'envs': n, 'calls_per_window': args.calls, 'rounds': args.rounds, 'us_per_call': {}}
  for pool in (True, False):
    env = BatchedEnv(n, seed=0, auto_reset=pool)
    acts = [torch.from_numpy(rs.randint(0, 17, n).astype(np.int32)).cuda() for _ in range(64)]
    masks = {'all': torch.ones(n, dtype=torch.uint8).cuda(), '1%': (torch.arange(n) % 100 == 0).to(torch.uint8).cuda()}
    env.reset()
    bank = WorldBank(env, **env.export_worlds(list(range(16))))
    res['objects_per_world'] = round(float(bank.nobj.mean()), 1)
    ids = torch.from_numpy(rs.randint(0, len(bank), n).astype(np.int32)).cuda()
    env.reset(worlds=bank, world_ids=ids)
    for t in range(args.warmup):
      env.step(acts[t % 64], info=False)
    torch.cuda.synchronize()

    def window(mask, authored):
      pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.calls)]
      for k, (a, b) in enumerate(pairs):
        for t in range(8):
          env.step(acts[(8 * k + t) % 64], info=False)
        a.record()
        if authored:
          env.reset(mask, worlds=bank, world_ids=ids)
        else:
          env.reset(mask)
        b.record()
      torch.cuda.synchronize()
      return [1e3 * a.elapsed_time(b) for a, b in pairs]

    for name, mask in masks.items():
      times = {'plain': [], 'worlds': []}
      for _ in range(args.rounds):
        times['plain'] += window(mask, False)
        times['worlds'] += window(mask, True)
      res['us_per_call'][f'{name}, pool {"on" if pool else "off"}'] = {
          k: {'median': round(float(np.median(v)), 1), 'mean': round(float(np.mean(v)), 1), 'p10': round(float(np.percentile(v, 10)), 1),
              'p90': round(float(np.percentile(v, 90)), 1)} for k, v in times.items()}
    env.check_errors()
    if pool:
      res['pool'] = env.pool_status()['state']
    del env
  print(json.dumps(res))
  if args.out:
    pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(args.out).write_text(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
  main()
