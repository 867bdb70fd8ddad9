#!/usr/bin/env python3
"""What an edit (BatchedEnv.edit) costs beside a step, on one GPU.  Not bench.py.

  python tools/edit_cost.py [--envs 4096] [--out profiles/edit_cost.json]

`--envs` envs of the default 64 x 64 world, `--burn-in` random steps into their episodes (auto-reset on), then in one process,
on one stream, alternated over `--rounds` rounds: `--calls` back-to-back calls between two HIP events of
  edit_1, edit_8, edit_64   edit(every env, a device tape of 1 / 8 / 64 ops per env)
  step                      step(info=False) on a tape of random actions
The tapes are built once, on the device, of ops that are valid in any state and leave the episodes playable -- SET_CELL of a
walkable material on a random cell (three in four ops), SET_ITEM of a resource, SET_PLAYER of a counter -- a different tape
for every env.  ADD / REMOVE / MOVE depend on the state and are not part of the tape: an op's own cost is a few LDS accesses
of one wave either way, what a call costs is the index check, the stage-in and the write-back.
The figure is device time per call with the launches queued ahead, i.e. the kernels' own time plus the gap between two
launches.  Every window is preceded by 50 unmeasured calls and ends in an event synchronise.  Medians over the rounds are
reported with each tape length's ratio to a step; every round is kept.
"""
import argparse
import json
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SEED, TAPE_SEED = 1000, 1234   # bench.py's convention
LENGTHS = (1, 8, 64)


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


def tape_of(env, n, length, rs):
  """int32 [n, length, 8] on the device: see the module's text."""
  from crafter_amd import abi
  rules = env.rules
  mats = [1 + list(rules['materials']).index(m) for m in ('grass', 'sand', 'path')]
  items = [list(rules['items']).index(i) for i in ('wood', 'stone', 'sapling')]
  t = np.zeros((n, length, 8), np.int32)
  kind = rs.randint(0, 8, size=(n, length))
  cell = kind < 6
  t[..., 0] = np.where(cell, abi.EDIT_SET_CELL, np.where(kind == 6, abi.EDIT_SET_ITEM, abi.EDIT_SET_PLAYER))
  t[..., 1] = np.where(cell, rs.randint(0, env.cfg.W, size=(n, length)), np.where(kind == 6, rs.choice(items, size=(n, length)), 1 + rs.randint(0, 2, size=(n, length))))
  t[..., 2] = np.where(cell, rs.randint(0, env.cfg.H, size=(n, length)), rs.randint(0, 10, size=(n, length)))
  t[..., 3] = np.where(cell, rs.choice(mats, size=(n, length)), 0)
  import torch
  return torch.from_numpy(t).to(env.device)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--envs', type=int, default=4096)
  ap.add_argument('--calls', type=int, default=1000)
  ap.add_argument('--burn-in', type=int, default=200)
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--out', default=str(ROOT / 'profiles' / 'edit_cost.json'))
  args = ap.parse_args()
  import torch
  from crafter_amd import BatchedEnv
  from crafter_amd.build import source_hash
  n = args.envs
  env = BatchedEnv(n, seed=SEED, auto_reset=True)
  rs = np.random.RandomState(TAPE_SEED)
  tape = torch.from_numpy(rs.randint(0, 17, size=(256, n)).astype(np.int32)).cuda()
  env.reset()
  clock = [0]

  def step():
    env.step(tape[clock[0] % tape.shape[0]], info=False)
    clock[0] += 1

  for _ in range(args.burn_in):
    step()
  idx = torch.arange(n, dtype=torch.int32, device=env.device)
  tapes = {length: tape_of(env, n, length, rs) for length in LENGTHS}
  calls = {f'edit_{length}': (lambda t=tapes[length]: env.edit(idx, t)) for length in LENGTHS}
  calls['step'] = step
  us = {k: [] for k in calls}
  for _ in range(args.rounds):
    for k, fn in calls.items():
      per_call(fn, 50)
      us[k].append(per_call(fn, args.calls))
  env.check_errors()
  med = {k: float(np.median(v)) for k, v in us.items()}
  doc = {'what': 'HIP events around `calls` back-to-back calls on one stream, device time per call in microseconds; medians over the rounds',
         'envs': n, 'calls': args.calls, 'burn_in': args.burn_in, 'rounds': args.rounds, 'seed': SEED, 'tape_seed': TAPE_SEED,
         'device': torch.cuda.get_device_name(0), 'csrc_sha16': source_hash(),
         'us_per_call': {k: [round(x, 3) for x in v] for k, v in us.items()},
         'us_per_call_median': {k: round(v, 3) for k, v in med.items()}}
  doc.update({f'edit_{length}_over_step': round(med[f'edit_{length}'] / med['step'], 4) for length in LENGTHS})
  out = pathlib.Path(args.out)
  out.parent.mkdir(parents=True, exist_ok=True)
  out.write_text(json.dumps(doc, indent=1) + '\n')
  print(json.dumps(doc))
  print(out)


if __name__ == '__main__':
  main()
