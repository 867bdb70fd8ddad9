#!/usr/bin/env python3
"""What a step of a subset of the batch (BatchedEnv.step_envs) costs, on one GPU.  Not bench.py.

  python tools/bench_step_envs.py [--out profiles/step_envs.json]

One process, the default geometry, a batch of 4096 envs with the world pool on, after a burn-in of random steps that leaves
the envs in ordinary mid-episode states.  Over `--rounds` rounds, alternating within each round, device time per call
(HIP events around `--calls` back-to-back calls, launches queued ahead: the kernels' own time plus the gaps between launches) of
  step            step() of the whole batch
  step_envs/n     step_envs(idx, actions) for n = 64, 512, 1024 and 4096, idx a fixed random subset on the device
  batch/n         step() of a separate batch of n envs (n = 64, 512, 1024): what the subset launch is measured against --
                  the gap is the one-workgroup index check in front of it
Every window ends in a device synchronise.  Medians over the rounds are reported, every round is kept;
pool_status()['regenerated_inline'] of the big batch before and after.  There is no CPU path: without a GPU the tool fails.
"""
import argparse
import json
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SEED, TAPE_SEED = 1000, 1234   # bench.py's convention
ENVS = 4096
SUBSETS = (64, 512, 1024, 4096)
TAPE = 64


def per_call(fn, calls):
  """-> microseconds of device time per call of fn(t) over `calls` back-to-back calls."""
  import torch
  start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  torch.cuda.synchronize()
  start.record()
  for t in range(calls):
    fn(t)
  end.record()
  end.synchronize()
  return 1e3 * start.elapsed_time(end) / calls


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--calls', type=int, default=300)
  ap.add_argument('--burn-in', type=int, default=300)
  ap.add_argument('--rounds', type=int, default=3)
  ap.add_argument('--out', default=str(ROOT / 'profiles' / 'step_envs.json'))
  args = ap.parse_args()
  import torch
  from crafter_amd import BatchedEnv
  from crafter_amd.build import source_hash
  rs = np.random.RandomState(TAPE_SEED)
  dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()
  env = BatchedEnv(ENVS, seed=SEED, auto_reset=True)
  env.reset()
  burn = dev(rs.randint(0, 17, (args.burn_in, ENVS)))
  for t in range(args.burn_in):
    env.step(burn[t], info=False)
  torch.cuda.synchronize()
  inline_before = env.pool_status()['regenerated_inline']
  tape = dev(rs.randint(0, 17, (TAPE, ENVS)))
  runs = {'step': lambda t: env.step(tape[t % TAPE], info=False)}
  keep = []
  for n in SUBSETS:
    idx = dev(rs.choice(ENVS, n, replace=False))
    acts = dev(rs.randint(0, 17, (TAPE, n)))
    keep.append((idx, acts))
    runs[f'step_envs/{n}'] = (lambda idx, acts: lambda t: env.step_envs(idx, acts[t % TAPE], info=False))(idx, acts)
  small = {}
  for n in SUBSETS[:-1]:
    b = BatchedEnv(n, seed=SEED, auto_reset=True)
    b.reset()
    acts = dev(rs.randint(0, 17, (TAPE, n)))
    for t in range(args.burn_in):
      b.step(acts[t % TAPE], info=False)
    small[n] = b
    runs[f'batch/{n}'] = (lambda b, acts: lambda t: b.step(acts[t % TAPE], info=False))(b, acts)
  for fn in runs.values():   # warm-up: scratch allocations, first launches
    per_call(fn, 20)
  us = {k: [] for k in runs}
  for _ in range(args.rounds):
    for k, fn in runs.items():
      us[k].append(per_call(fn, args.calls))
  env.check_errors()
  for b in small.values():
    b.check_errors()
  med = {k: float(np.median(v)) for k, v in us.items()}
  doc = {
      'what': 'HIP events around `calls` back-to-back calls, device time per call in microseconds; step: step() of the 4096-env batch; '
              'step_envs/n: step_envs of a fixed random subset of n of its envs; batch/n: step() of a separate n-env batch',
      'envs': ENVS, 'calls': args.calls, 'burn_in': args.burn_in, 'rounds': args.rounds, 'seed': SEED, 'tape_seed': TAPE_SEED,
      'device': torch.cuda.get_device_name(0), 'csrc_sha16': source_hash(), 'step_instance': env.step_instance,
      'us_per_call': {k: [round(x, 3) for x in v] for k, v in us.items()},
      'us_per_call_median': {k: round(v, 3) for k, v in med.items()},
      'step_envs_over_step': {str(n): round(med[f'step_envs/{n}'] / med['step'], 4) for n in SUBSETS},
      'step_envs_minus_batch_us': {str(n): round(med[f'step_envs/{n}'] - med[f'batch/{n}'], 3) for n in SUBSETS[:-1]},
      'regenerated_inline': {'before': inline_before, 'after': env.pool_status()['regenerated_inline']},
      'pool': env.pool_status(stats=False)['state'],
  }
  out = pathlib.Path(args.out)
  out.parent.mkdir(parents=True, exist_ok=True)
  out.write_text(json.dumps(doc, indent=1) + '\n')
  print(json.dumps(doc))
  print(out)
  if not med['step_envs/64'] < med['step']:
    sys.exit(f'step_envs of 64 envs ({med["step_envs/64"]:.1f} us) is not below step() of {ENVS} ({med["step"]:.1f} us)')


if __name__ == '__main__':
  main()
