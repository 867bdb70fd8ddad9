#!/usr/bin/env python3
"""What an audit of every row (BatchedEnv.audit) costs beside a step, on one GPU.  Not bench.py.

  python tools/audit_cost.py [--out profiles/audit_cost.json]

Two batches, one after the other in one process: `--envs` envs of the default 64 x 64 world (the audit's one-wave instance) and
`--large-envs` envs of 256 x 256 cells (a workgroup per env, objmap audited).  Each is played `--burn-in` random steps into its
episodes (auto-reset on); then, on one stream, alternated over `--rounds` rounds: `--calls` back-to-back calls between two HIP
events of
  audit           audit(out=)
  fingerprint     fingerprint(out=), the sibling read-only kernel that reads the same row
  step            step(info=False) on a tape of random actions (its state moves on: the audits of the next round see later states)
The figure is device time per call with the launches queued ahead, i.e. the kernel's own time plus the gap between two
launches.  Every window is preceded by `--warmup` unmeasured calls and ends in an event synchronise.  Medians over the rounds
are reported with their spread ((max - min) / median) and the ratio a reader needs, audit / step: "an audit costs x steps".
Every round is kept.  The flags of the last audit are read back: a cost measured on rows that fail would be another cost.
"""
import argparse
import json
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SEED, TAPE_SEED = 1000, 1234   # bench.py's convention


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
  out = torch.zeros(n, dtype=torch.int32, device='cuda'), torch.zeros((n, 4), dtype=torch.int32, device='cuda')
  key = torch.zeros(n, dtype=torch.int64, device='cuda')
  fns = {'audit': lambda: env.audit(out=out), 'fingerprint': lambda: env.fingerprint(out=key), 'step': step}
  us = {k: [] for k in fns}
  for _ in range(args.rounds):
    for k, fn in fns.items():
      per_call(fn, args.warmup)
      us[k].append(per_call(fn, calls))
  env.audit(out=out)
  failing = int((out[0] != 0).sum())
  env.check_errors()
  med = {k: float(np.median(v)) for k, v in us.items()}
  return {'envs': n, 'area': list(area), 'calls': calls, 'steps_played': clock[0], 'rows_failing': failing,
          'audit_instance': 'one wave per env' if area[0] * area[1] <= 4096 else 'one workgroup of 256 threads per env',
          'us_per_call': {k: [round(x, 3) for x in v] for k, v in us.items()},
          'us_per_call_median': {k: round(v, 3) for k, v in med.items()},
          'spread': {k: round((max(v) - min(v)) / med[k], 4) for k, v in us.items()},
          'audit_over_step': round(med['audit'] / med['step'], 4),
          'audit_over_fingerprint': round(med['audit'] / med['fingerprint'], 4)}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--envs', type=int, default=4096)
  ap.add_argument('--large-envs', type=int, default=8192)
  ap.add_argument('--calls', type=int, default=300)
  ap.add_argument('--large-calls', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=20)
  ap.add_argument('--burn-in', type=int, default=200)
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--out', default=str(ROOT / 'profiles' / 'audit_cost.json'))
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
