#!/usr/bin/env python3
"""What the symbolic observation (BatchedEnv.symbolic) costs and what it gains, on one GPU.  Not bench.py.

  python tools/bench_symbolic.py loops --out build/symbolic_obs/loops.json
      At each batch size, three closed loops on the same box in the same process, alternated over `--rounds` rounds, each
      window `--steps` steady-state steps with no host synchronisation inside:
        a  step() with render=True                 (the loop of a pixel learner)
        b  step() with render=False
        c  step() with render=False + symbolic()   (the loop of a symbolic learner)
      c / b is the price of the feature, c / a what a symbolic learner gains over pixels.
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_symbolic.py trace
      Loop c alone at 4096 envs, for the kernels' own times (crafter_symbolic_kernel beside crafter_rules_kernel).
  python tools/bench_symbolic.py merge --loops build/symbolic_obs/loops.json --stats DIR
      -> profiles/symbolic_obs.json: the loops, the trace's crafter kernels and the source hash.
"""
import argparse
import csv
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SEED, TAPE_SEED = 1000, 1234   # bench.py's convention


def make(envs, render):
  from crafter_amd import BatchedEnv
  return BatchedEnv(envs, seed=SEED, auto_reset=True, render=render)


def window(env, tape, t0, steps, symbolic, out):
  import torch
  torch.cuda.synchronize()
  start = time.perf_counter()
  for t in range(t0, t0 + steps):
    env.step(tape[t % tape.shape[0]], info=False)
    if symbolic:
      env.symbolic(out=out)
  torch.cuda.synchronize()
  return steps * env.num_envs / (time.perf_counter() - start)


def loops(args):
  import torch
  res = {}
  for envs in args.envs:
    tape = torch.from_numpy(np.random.RandomState(TAPE_SEED).randint(0, 17, size=(args.burn_in + args.steps, envs)).astype(np.int32)).cuda()
    batch = {'a': make(envs, True), 'b': make(envs, False), 'c': make(envs, False)}
    ls, ss = batch['c'].symbolic_shape
    out = (torch.zeros((envs,) + ls, dtype=torch.uint8, device='cuda'), torch.zeros((envs,) + ss, dtype=torch.float32, device='cuda'))
    pos = {}
    for k, env in batch.items():
      env.reset()
      window(env, tape, 0, args.burn_in, k == 'c', out)
      pos[k] = args.burn_in
    rates = {k: [] for k in batch}
    for _ in range(args.rounds):
      for k, env in batch.items():
        rates[k].append(window(env, tape, pos[k], args.steps, k == 'c', out))
        pos[k] += args.steps
    for env in batch.values():
      env.check_errors()
    med = {k: float(np.median(v)) for k, v in rates.items()}
    res[str(envs)] = {
        'env_steps_per_s': {k: [round(x) for x in v] for k, v in rates.items()}, 'median': {k: round(v) for k, v in med.items()},
        'us_per_step': {k: round(1e6 * envs / v, 2) for k, v in med.items()},
        'c_over_b': round(med['c'] / med['b'], 4), 'c_over_a': round(med['c'] / med['a'], 4),
        'symbolic_us_per_call_from_loops': round(1e6 * envs * (1 / med['c'] - 1 / med['b']), 2),
        'bytes_out_per_env': int(np.prod(ls)) + 4 * int(np.prod(ss)), 'frame_bytes_per_env': int(np.prod(batch['a'].obs.shape[1:]))}
    print(json.dumps({envs: res[str(envs)]}), flush=True)
    del batch
  doc = {'loops': {'a': 'step(), render=True', 'b': 'step(), render=False', 'c': 'step(), render=False + symbolic(out=)'},
         'steps_per_window': args.steps, 'burn_in': args.burn_in, 'rounds': args.rounds, 'seed': SEED, 'tape_seed': TAPE_SEED,
         'device': torch.cuda.get_device_name(0), 'results': res}
  return doc


def trace(args):
  import torch
  env = make(args.trace_envs, False)
  tape = torch.from_numpy(np.random.RandomState(TAPE_SEED).randint(0, 17, size=(64, args.trace_envs)).astype(np.int32)).cuda()
  env.reset()
  out = env.symbolic()
  window(env, tape, 0, args.trace_steps, True, out)
  env.check_errors()
  return {'envs': args.trace_envs, 'steps': args.trace_steps}


def short(name):
  name = name.replace('(anonymous namespace)::', '').split('(')[0]
  return name[5:] if name.startswith('void ') else name


def merge(args):
  from crafter_amd.build import source_hash
  doc = json.loads(pathlib.Path(args.loops).read_text())
  hits = sorted(pathlib.Path(args.stats).rglob('*kernel_stats.csv'))
  if not hits:
    raise SystemExit(f'no *kernel_stats.csv under {args.stats}')
  kernels = {}
  for r in csv.DictReader(open(hits[0])):
    if 'crafter' in r['Name']:
      kernels[short(r['Name'])] = {'calls': int(r['Calls']), 'average_ns': float(r['AverageNs']), 'min_ns': float(r['MinNs']),
                                   'max_ns': float(r['MaxNs']), 'percentage': float(r['Percentage'])}
  doc['kernel_trace'] = {'what': f'rocprofv3 --kernel-trace --stats of loop c alone at {args.trace_envs} envs, {args.trace_steps} steps',
                         'kernels': kernels}
  doc['csrc_sha16'] = source_hash()
  out = ROOT / 'profiles' / 'symbolic_obs.json'
  out.write_text(json.dumps(doc, indent=1) + '\n')
  print(out)
  return doc


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('mode', choices=('loops', 'trace', 'merge'))
  ap.add_argument('--envs', type=int, nargs='+', default=[4096, 16384])
  ap.add_argument('--steps', type=int, default=2000)
  ap.add_argument('--burn-in', type=int, default=400)
  ap.add_argument('--rounds', type=int, default=3)
  ap.add_argument('--trace-envs', type=int, default=4096)
  ap.add_argument('--trace-steps', type=int, default=600)
  ap.add_argument('--loops', default='build/symbolic_obs/loops.json')
  ap.add_argument('--stats', default='build/symbolic_obs/stats')
  ap.add_argument('--out', default='')
  args = ap.parse_args()
  res = {'loops': loops, 'trace': trace, 'merge': merge}[args.mode](args)
  if args.out:
    pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(args.out).write_text(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
  main()
