#!/usr/bin/env python3
"""What an open-loop rollout of a subset of the batch (BatchedEnv.rollout_envs) costs, on one GPU.  Not bench.py.

  python tools/bench_rollout_envs.py [--out profiles/rollout_envs.json]

One process, the default geometry, a batch of 4096 envs with the world pool on and frames drawn, after a burn-in of random
steps that leaves the envs in ordinary mid-episode states.  For n = 16, 256 and 1024 named envs (a fixed random subset, on the
device) and T = 16 steps, over `--reps` repetitions, alternating within each repetition, device time per env-step (HIP events
around `--calls` back-to-back windows, launches queued ahead: the kernels' own time plus the gaps between launches) of
  rollout_envs/n  one rollout_envs(idx, actions[T, n]) per window
  step_envs/n     T step_envs(idx, actions[t]) calls per window over the same idx: the yardstick
  rollout/n       one rollout(actions[T, n]) per window on a separate batch of n envs
Every measurement ends in a device synchronise.  Minimum and maximum over the repetitions are reported, every repetition is
kept; pool_status()['regenerated_inline'] of the big batch before and after.  There is no CPU path: without a GPU the tool fails.
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
SUBSETS = (16, 256, 1024)
T = 16
TAPES = 4


def per_window(fn, calls):
  """-> microseconds of device time per call of fn(k) over `calls` back-to-back calls."""
  import torch
  start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  torch.cuda.synchronize()
  start.record()
  for k in range(calls):
    fn(k)
  end.record()
  end.synchronize()
  return 1e3 * start.elapsed_time(end) / calls


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--calls', type=int, default=500, help='windows of T steps per measurement')
  ap.add_argument('--burn-in', type=int, default=300)
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--out', default=str(ROOT / 'profiles' / 'rollout_envs.json'))
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
  runs, small = {}, {}
  for n in SUBSETS:
    idx = dev(rs.choice(ENVS, n, replace=False))
    acts = dev(rs.randint(0, 17, (TAPES, T, n)))
    out = (torch.empty((T, n) + tuple(env.obs.shape[1:]), dtype=torch.uint8, device='cuda'),
           torch.empty((T, n), dtype=torch.float32, device='cuda'), torch.empty((T, n), dtype=torch.uint8, device='cuda'))

    def subset_rollout(k, idx=idx, acts=acts, out=out):
      env.rollout_envs(idx, acts[k % TAPES], out=out)

    def subset_steps(k, idx=idx, acts=acts):
      a = acts[k % TAPES]
      for t in range(T):
        env.step_envs(idx, a[t], info=False)

    b = BatchedEnv(n, seed=SEED, auto_reset=True)
    b.reset()
    for t in range(args.burn_in):
      b.step(acts[t % TAPES, t % T], info=False)
    small[n] = b
    out_b = tuple(torch.empty_like(x) for x in out)

    def batch_rollout(k, b=b, acts=acts, out=out_b):
      b.rollout(acts[k % TAPES], out=out)

    runs[f'rollout_envs/{n}'] = (subset_rollout, n)
    runs[f'step_envs/{n}'] = (subset_steps, n)
    runs[f'rollout/{n}'] = (batch_rollout, n)
  for fn, _ in runs.values():   # warm-up: scratch allocations, first launches
    per_window(fn, 5)
  ns = {k: [] for k in runs}    # nanoseconds per env-step
  for _ in range(args.reps):
    for k, (fn, n) in runs.items():
      ns[k].append(1e3 * per_window(fn, args.calls) / (T * n))
  env.check_errors()
  for b in small.values():
    b.check_errors()
  doc = {
      'what': 'HIP events around `calls` back-to-back windows of T steps of n envs, device time in nanoseconds per env-step; '
              'rollout_envs/n: one rollout_envs call over a fixed random subset of n envs of the 4096-env batch; step_envs/n: T step_envs '
              'calls over the same subset; rollout/n: rollout() of a separate n-env batch',
      'envs': ENVS, 'T': T, 'calls': args.calls, 'burn_in': args.burn_in, 'reps': args.reps, 'seed': SEED, 'tape_seed': TAPE_SEED,
      'device': torch.cuda.get_device_name(0), 'csrc_sha16': source_hash(), 'step_instance': env.step_instance,
      'ns_per_env_step': {k: [round(x, 2) for x in v] for k, v in ns.items()},
      'ns_per_env_step_min_max': {k: [round(min(v), 2), round(max(v), 2)] for k, v in ns.items()},
      'regenerated_inline': {'before': inline_before, 'after': env.pool_status()['regenerated_inline']},
      'pool': env.pool_status(stats=False)['state'],
  }
  out = pathlib.Path(args.out)
  out.parent.mkdir(parents=True, exist_ok=True)
  out.write_text(json.dumps(doc, indent=1) + '\n')
  print(json.dumps(doc))
  print(f'{"n":>6} {"rollout_envs":>22} {"T x step_envs":>22} {"rollout (n-env batch)":>24}   ns per env-step, min - max of {args.reps}')
  for n in SUBSETS:
    cells = ['%.1f - %.1f' % (min(ns[f'{k}/{n}']), max(ns[f'{k}/{n}'])) for k in ('rollout_envs', 'step_envs', 'rollout')]
    print(f'{n:>6} {cells[0]:>22} {cells[1]:>22} {cells[2]:>24}')
  print(out)


if __name__ == '__main__':
  main()
