#!/usr/bin/env python3
"""What the legal-action mask (BatchedEnv.legal_actions) costs, on one GPU.  Not bench.py.

  python tools/bench_legal_actions.py [--out profiles/legal_actions.json]

For each configuration -- 4096 and 16384 envs of the default 64 x 64 world (the slot-table path, MAP 0) and 8192 envs of a
256 x 256 world (the objmap path, MAP 1) -- in one process, after a burn-in of random steps that leaves the envs in ordinary
mid-episode states:
  per call    `--calls` back-to-back legal_actions(out=) between two HIP events, and the same for symbolic(out=) (the sibling
              kernel over the same records, unchanged by this feature), alternated over `--rounds` rounds; the figure is device
              time per call with the launches queued ahead, i.e. the kernel's own time plus the gap between two launches
  closed loop `--steps` steps of step(render=False) with and without one legal_actions(out=) per step, no host synchronisation
              inside a window, alternated over `--rounds` rounds; the difference of the step periods is what a mask-aware learner
              pays per step
Every window ends in a device synchronise.  Medians over the rounds are reported, every round is kept.
"""
import argparse
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SEED, TAPE_SEED = 1000, 1234   # bench.py's convention
CONFIGS = (('4096', 4096, (64, 64)), ('16384', 16384, (64, 64)), ('8192x256x256', 8192, (256, 256)))


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


def loop(env, tape, t0, steps, legal_out):
  """-> microseconds per step of a closed loop window."""
  import torch
  torch.cuda.synchronize()
  start = time.perf_counter()
  for t in range(t0, t0 + steps):
    env.step(tape[t % tape.shape[0]], info=False)
    if legal_out is not None:
      env.legal_actions(out=legal_out)
  torch.cuda.synchronize()
  return 1e6 * (time.perf_counter() - start) / steps


def measure(envs, area, args):
  import torch
  from crafter_amd import BatchedEnv
  tape = torch.from_numpy(np.random.RandomState(TAPE_SEED).randint(0, 17, size=(args.burn_in + args.steps, envs)).astype(np.int32)).cuda()
  batch = {k: BatchedEnv(envs, seed=SEED, area=area, auto_reset=True, render=False) for k in ('plain', 'masked')}
  legal = torch.zeros((envs, batch['masked'].num_actions), dtype=torch.uint8, device='cuda')
  ls, ss = batch['masked'].symbolic_shape
  sym = (torch.zeros((envs,) + ls, dtype=torch.uint8, device='cuda'), torch.zeros((envs,) + ss, dtype=torch.float32, device='cuda'))
  pos = {}
  for k, env in batch.items():
    env.reset()
    loop(env, tape, 0, args.burn_in, legal if k == 'masked' else None)
    pos[k] = args.burn_in
  env = batch['masked']
  calls = {'legal_actions': lambda: env.legal_actions(out=legal), 'symbolic': lambda: env.symbolic(out=sym)}
  for fn in calls.values():
    per_call(fn, 50)
  call_us = {k: [] for k in calls}
  for _ in range(args.rounds):
    for k, fn in calls.items():
      call_us[k].append(per_call(fn, args.calls))
  step_us = {k: [] for k in batch}
  for _ in range(args.rounds):
    for k, e in batch.items():
      step_us[k].append(loop(e, tape, pos[k], args.steps, legal if k == 'masked' else None))
      pos[k] += args.steps
  for e in batch.values():
    e.check_errors()
  med = lambda v: float(np.median(v))
  res = {
      'envs': envs, 'area': list(area), 'slot_map_derived': bool(env.slot_map_derived), 'step_instance': env.step_instance,
      'us_per_call': {k: [round(x, 3) for x in v] for k, v in call_us.items()},
      'us_per_call_median': {k: round(med(v), 3) for k, v in call_us.items()},
      'legal_over_symbolic': round(med(call_us['legal_actions']) / med(call_us['symbolic']), 4),
      'us_per_step': {k: [round(x, 2) for x in v] for k, v in step_us.items()},
      'us_per_step_median': {k: round(med(v), 2) for k, v in step_us.items()},
      'masked_over_plain': round(med(step_us['masked']) / med(step_us['plain']), 4),
      'legal_us_per_step_from_loops': round(med(step_us['masked']) - med(step_us['plain']), 2),
      'legal_fraction': round(float(legal.float().mean()), 4),
      'bytes_out_per_env': {'legal_actions': int(legal.shape[1]), 'symbolic': int(np.prod(ls)) + 4 * int(np.prod(ss))}}
  del batch
  return res


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--configs', nargs='+', default=[c[0] for c in CONFIGS], choices=[c[0] for c in CONFIGS])
  ap.add_argument('--calls', type=int, default=2000)
  ap.add_argument('--steps', type=int, default=1000)
  ap.add_argument('--burn-in', type=int, default=300)
  ap.add_argument('--rounds', type=int, default=3)
  ap.add_argument('--out', default=str(ROOT / 'profiles' / 'legal_actions.json'))
  args = ap.parse_args()
  import torch
  from crafter_amd.build import source_hash
  out = pathlib.Path(args.out)
  out.parent.mkdir(parents=True, exist_ok=True)
  doc = {'what': {'us_per_call': 'HIP events around `calls` back-to-back calls (out= given), device time per call',
                  'us_per_step': 'closed loop of step(render=False), `plain`, and the same + one legal_actions(out=) per step, `masked`'},
         'calls': args.calls, 'steps_per_window': args.steps, 'burn_in': args.burn_in, 'rounds': args.rounds, 'seed': SEED,
         'tape_seed': TAPE_SEED, 'device': torch.cuda.get_device_name(0), 'results': {}, 'csrc_sha16': source_hash()}
  for name, envs, area in CONFIGS:
    if name in args.configs:
      doc['results'][name] = measure(envs, area, args)
      print(json.dumps({name: doc['results'][name]}), flush=True)
      out.write_text(json.dumps(doc, indent=1) + '\n')   # after every configuration: a run cut short keeps what it measured
  print(out)


if __name__ == '__main__':
  main()
