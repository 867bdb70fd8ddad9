#!/usr/bin/env python3
"""What a navigation query (BatchedEnv.navigate) costs beside a step, on one GPU.  Not bench.py.

  python tools/navigate_cost.py [--envs 4096] [--out profiles/navigate_cost.json]

`--envs` envs of the default 64 x 64 world, `--burn-in` random steps into their episodes (auto-reset on), then in one process,
on one stream, alternated over `--rounds` rounds: `--calls` back-to-back calls between two HIP events of
  navigate_k1     navigate(['tree'], out=)
  navigate_k8     navigate(eight targets, out=)
  legal_actions   legal_actions(out=), the sibling read-only kernel
  step            step(info=False) on a tape of random actions (its state moves on: the queries in the next round see later states)
The figure is device time per call with the launches queued ahead, i.e. the kernel's own time plus the gap between two
launches.  Every window is preceded by 50 unmeasured calls and ends in an event synchronise.  Medians over the rounds are
reported with the two ratios a reader needs -- navigate_k8 / step and navigate_k8 / legal_actions --, every round is kept.
"""
import argparse
import json
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SEED, TAPE_SEED = 1000, 1234   # bench.py's convention
K8 = ['tree', 'water', 'cow', 'table', 'stone', ['coal', 'iron'], 'diamond', 'zombie']


def per_call(fn, calls):
  """-> microseconds of device time per call of fn over `calls` back-to-back calls."""
  import torch
  start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  torch.cuda.synchronize()
  start.record()
  for _ in range(calls):
    fn()
  end.record()
  end.synchronize()
  return 1e3 * start.elapsed_time(end) / calls


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--envs', type=int, default=4096)
  ap.add_argument('--calls', type=int, default=1000)
  ap.add_argument('--burn-in', type=int, default=200)
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--out', default=str(ROOT / 'profiles' / 'navigate_cost.json'))
  args = ap.parse_args()
  import torch
  from crafter_amd import BatchedEnv
  from crafter_amd.build import source_hash
  n = args.envs
  env = BatchedEnv(n, seed=SEED, auto_reset=True)
  tape = torch.from_numpy(np.random.RandomState(TAPE_SEED).randint(0, 17, size=(256, n)).astype(np.int32)).cuda()
  env.reset()
  clock = [0]

  def step():
    env.step(tape[clock[0] % tape.shape[0]], info=False)
    clock[0] += 1

  for _ in range(args.burn_in):
    step()
  new = lambda k: tuple(torch.zeros((n, k), dtype=dt, device='cuda') for dt in (torch.int32, torch.int32, torch.uint8))
  out1, out8 = new(1), new(len(K8))
  legal = torch.zeros((n, env.num_actions), dtype=torch.uint8, device='cuda')
  calls = {'navigate_k1': lambda: env.navigate(['tree'], out=out1), 'navigate_k8': lambda: env.navigate(K8, out=out8),
           'legal_actions': lambda: env.legal_actions(out=legal), 'step': step}
  us = {k: [] for k in calls}
  for _ in range(args.rounds):
    for k, fn in calls.items():
      per_call(fn, 50)
      us[k].append(per_call(fn, args.calls))
  env.check_errors()
  med = {k: float(np.median(v)) for k, v in us.items()}
  dist = out8[0]
  doc = {'what': 'HIP events around `calls` back-to-back calls on one stream, device time per call in microseconds; medians over the rounds',
         'envs': n, 'calls': args.calls, 'burn_in': args.burn_in, 'rounds': args.rounds, 'seed': SEED, 'tape_seed': TAPE_SEED,
         'device': torch.cuda.get_device_name(0), 'csrc_sha16': source_hash(), 'targets_k8': [str(t) for t in K8],
         'us_per_call': {k: [round(x, 3) for x in v] for k, v in us.items()},
         'us_per_call_median': {k: round(v, 3) for k, v in med.items()},
         'navigate_k8_over_step': round(med['navigate_k8'] / med['step'], 4),
         'navigate_k8_over_legal_actions': round(med['navigate_k8'] / med['legal_actions'], 4),
         'navigate_k1_over_step': round(med['navigate_k1'] / med['step'], 4),
         'k8_dist': {'unreachable_fraction': round(float((dist < 0).float().mean()), 4), 'mean_reachable': round(float(dist[dist > 0].float().mean()), 2),
                     'max': int(dist.max())}}
  out = pathlib.Path(args.out)
  out.parent.mkdir(parents=True, exist_ok=True)
  out.write_text(json.dumps(doc, indent=1) + '\n')
  print(json.dumps(doc))
  print(out)


if __name__ == '__main__':
  main()
