#!/usr/bin/env python3
"""What a nearby query (BatchedEnv.nearby) costs beside a step, on one GPU.  Not bench.py.

  python tools/nearby_cost.py [--out profiles/nearby_cost.json]

Two batches, one after the other in one process: `--envs` envs of the default 64 x 64 world (the query's one-wave instance, the
slot table) and `--large-envs` envs of 256 x 256 cells (a workgroup per env, objmap where the window is short).  Each is played
`--burn-in` random steps into its episodes (auto-reset on); then, on one stream, alternated over `--rounds` rounds: `--calls`
back-to-back calls between two HIP events of
  nearby_d4       nearby(4, k=16, out=): a 9 x 9 window, the 16 nearest creatures
  nearby_world    nearby(None, k=16, out=): the whole world's census, the 16 nearest creatures of all
  census          nearby(None, k=0, out=): the census alone (what count() calls)
  legal_actions   legal_actions(out=), the sibling read-only kernel
  step            step(info=False) on a tape of random actions (its state moves on: the queries of the next round see later states)
The figure is device time per call with the launches queued ahead, i.e. the kernel's own time plus the gap between two
launches.  Every window is preceded by `--warmup` unmeasured calls and ends in an event synchronise.  Medians over the rounds
are reported with their spread ((max - min) / median) and the ratios a reader needs, each query / step: "a query costs x steps".
Every round is kept.  The last whole-world answer is read back: how many objects qualified per env, and how many envs had more
than k.
"""
import argparse
import json
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SEED, TAPE_SEED = 1000, 1234   # bench.py's convention
K = 16


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


def measure(n, area, args, calls):
  import torch
  from crafter_amd import BatchedEnv
  env = BatchedEnv(n, area=area, seed=SEED, auto_reset=True)
  tape = torch.from_numpy(np.random.RandomState(TAPE_SEED).randint(0, 17, size=(256, n)).astype(np.int32)).cuda()
  env.reset()
  clock = [0]

  def step():
    env.step(tape[clock[0] % tape.shape[0]], info=False)
    clock[0] += 1

  for _ in range(args.burn_in):
    step()
  ncls = len(env.symbolic_names['classes'])
  new = lambda k: (torch.zeros((n, ncls), dtype=torch.int32, device='cuda'), torch.zeros((n, k, 6), dtype=torch.int16, device='cuda'),
                   torch.zeros(n, dtype=torch.int32, device='cuda'))
  out_d4, out_world, out_census = new(K), new(K), new(0)
  legal = torch.zeros((n, env.num_actions), dtype=torch.uint8, device='cuda')
  fns = {'nearby_d4': lambda: env.nearby(4, K, out=out_d4), 'nearby_world': lambda: env.nearby(None, K, out=out_world),
         'census': lambda: env.nearby(None, 0, out=out_census), 'legal_actions': lambda: env.legal_actions(out=legal), 'step': step}
  us = {k: [] for k in fns}
  for _ in range(args.rounds):
    for k, fn in fns.items():
      per_call(fn, args.warmup)
      us[k].append(per_call(fn, calls))
  env.nearby(None, K, out=out_world)
  env.nearby(4, K, out=out_d4)
  env.check_errors()
  med = {k: float(np.median(v)) for k, v in us.items()}
  return {'envs': n, 'area': list(area), 'calls': calls, 'k': K, 'steps_played': clock[0],
          'instance': 'one wave per env' if max(area) <= 64 else 'one workgroup of 256 threads per env',
          'qualified_world_mean': round(float(out_world[2].float().mean()), 2), 'qualified_world_above_k': int((out_world[2] > K).sum()),
          'qualified_d4_mean': round(float(out_d4[2].float().mean()), 3),
          'us_per_call': {k: [round(x, 3) for x in v] for k, v in us.items()},
          'us_per_call_median': {k: round(v, 3) for k, v in med.items()},
          'spread': {k: round((max(v) - min(v)) / med[k], 4) for k, v in us.items()},
          'nearby_d4_over_step': round(med['nearby_d4'] / med['step'], 4),
          'nearby_world_over_step': round(med['nearby_world'] / med['step'], 4),
          'census_over_step': round(med['census'] / med['step'], 4),
          'nearby_d4_over_legal_actions': round(med['nearby_d4'] / med['legal_actions'], 4)}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--envs', type=int, default=4096)
  ap.add_argument('--large-envs', type=int, default=8192)
  ap.add_argument('--calls', type=int, default=300)
  ap.add_argument('--large-calls', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=20)
  ap.add_argument('--burn-in', type=int, default=200)
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--out', default=str(ROOT / 'profiles' / 'nearby_cost.json'))
  args = ap.parse_args()
  import torch
  from crafter_amd.build import source_hash
  doc = {'what': 'HIP events around `calls` back-to-back calls on one stream, device time per call in microseconds; medians over the rounds, '
                 'spread = (max - min) / median',
         'warmup': args.warmup, 'burn_in': args.burn_in, 'rounds': args.rounds, 'seed': SEED, 'tape_seed': TAPE_SEED,
         'device': torch.cuda.get_device_name(0), 'csrc_sha16': source_hash(),
         'default': measure(args.envs, (64, 64), args, args.calls)}
  if args.large_envs > 0:
    doc['large'] = measure(args.large_envs, (256, 256), args, args.large_calls)
  out = pathlib.Path(args.out)
  out.parent.mkdir(parents=True, exist_ok=True)
  out.write_text(json.dumps(doc, indent=1) + '\n')
  print(json.dumps(doc))
  print(out)


if __name__ == '__main__':
  main()
