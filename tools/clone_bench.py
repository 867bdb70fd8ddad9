#!/usr/bin/env python3
"""Cost of copying environments (BatchedEnv.copy_envs) at the headline geometry (64x64, pool on).  Not bench.py.

  python tools/clone_bench.py kernel   # copies only: run under rocprofv3 --kernel-trace --stats for the kernel time;
                                       # prints the bytes one call moves (read + written, from state.state_spec)
  python tools/clone_bench.py loop     # (b) closed-loop env-steps/s with one copy_envs of 512 pairs every 8 steps against
                                       # the same loop without copies, alternated in one process; pool on and gen_period=-1

TB/s of the copy kernel = bytes of one call / its mean time in the rocprofv3 stats of the `kernel` run."""
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


def pair_bytes(env):
  """Bytes one pair of crafter_copy_envs reads (= writes): the rows of env_copy.hpp make_copy_plan."""
  cfg = env.cfg
  spec = state.store_spec(cfg, 1, env.slot_map_derived)
  row = sum(int(np.prod(shape[1:])) * np.dtype(dt).itemsize for shape, dt in spec.values())
  if 'pool_hdr' in env.state:
    full = state.state_spec(cfg)
    for name in ('pool_mat', 'pool_objs', 'pool_mt', 'pool_hdr', 'pool_chunk_order', 'pool_perm', 'pool_census'):
      shape, dt = full[name]
      row += 2 * int(np.prod(shape[2:])) * np.dtype(dt).itemsize
    row += 4   # gen_latest
  return row


def warm(env, steps, rs):
  env.reset()
  for _ in range(steps):
    env.step(torch.from_numpy(rs.randint(0, 17, env.num_envs).astype(np.int32)).to(env.device), info=False)
  torch.cuda.synchronize()


def kernel(args):
  rs = np.random.RandomState(0)
  out = []
  for envs, pairs in ((2 * args.pairs_big, args.pairs_big), (4096, 512)):
    env = BatchedEnv(envs, seed=0, length=args.length)
    warm(env, 40, rs)
    perm = rs.permutation(envs)
    src = torch.from_numpy(perm[:pairs].astype(np.int32)).cuda()
    dst = torch.from_numpy(perm[pairs:2 * pairs].astype(np.int32)).cuda()
    for _ in range(args.reps):
      env.copy_envs(src, dst)
    torch.cuda.synchronize()
    env.check_errors()
    b = pair_bytes(env)
    out.append({'envs': envs, 'pairs': pairs, 'calls': args.reps, 'bytes_per_pair_read': b,
                'bytes_per_call_read_plus_written': 2 * b * pairs})
    del env
  for r in out:
    print(json.dumps(r))
  return out


def loop(args):
  rs = np.random.RandomState(1)
  res = {}
  for gen_period in (0, -1):
    env = BatchedEnv(4096, seed=0, length=args.length, gen_period=gen_period)
    acts = [torch.from_numpy(rs.randint(0, 17, 4096).astype(np.int32)).cuda() for _ in range(64)]
    perm = rs.permutation(4096)
    src = torch.from_numpy(perm[:512].astype(np.int32)).cuda()
    dst = torch.from_numpy(perm[512:1024].astype(np.int32)).cuda()
    warm(env, args.warmup, rs)

    def window(copies):
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      for t in range(args.steps):
        if copies and t % 8 == 7:
          env.copy_envs(src, dst)
        env.step(acts[t % 64], info=False)
      torch.cuda.synchronize()
      return args.steps * 4096 / (time.perf_counter() - t0)

    rates = {'plain': [], 'copy_every_8': []}
    for _ in range(args.rounds):
      rates['plain'].append(window(False))
      rates['copy_every_8'].append(window(True))
    env.check_errors()
    key = 'pool_on' if gen_period == 0 else 'gen_period_-1'
    med = {k: float(np.median(v)) for k, v in rates.items()}
    step_us = 1e6 * 4096 / med['plain']
    # extra time per copy call = (time per 8 steps with a copy - time per 8 steps without)
    per_copy_us = 8 * 4096 * (1 / med['copy_every_8'] - 1 / med['plain']) * 1e6
    res[key] = {'env_steps_per_s': {k: [round(x) for x in v] for k, v in rates.items()}, 'median': {k: round(v) for k, v in med.items()},
                'step_us': round(step_us, 1), 'extra_us_per_copy_call': round(per_copy_us, 1)}
    del env
  print(json.dumps(res))
  return res


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('mode', choices=('kernel', 'loop'))
  ap.add_argument('--reps', type=int, default=50)
  ap.add_argument('--pairs-big', type=int, default=4096)
  ap.add_argument('--length', type=int, default=10000)
  ap.add_argument('--steps', type=int, default=800)
  ap.add_argument('--warmup', type=int, default=200)
  ap.add_argument('--rounds', type=int, default=3)
  ap.add_argument('--out', default='')
  args = ap.parse_args()
  res = kernel(args) if args.mode == 'kernel' else loop(args)
  if args.out:
    pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(args.out).write_text(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
  main()
