#!/usr/bin/env python3
"""What a state fingerprint (BatchedEnv.fingerprint / fingerprint_parts) costs, on one GPU.  Not bench.py.

  python tools/fingerprint_bench.py [--out profiles/fingerprint.json]

For each configuration -- 4096 envs of the default 64 x 64 world and BASELINE configs[3], 8192 envs of a 256 x 256 world -- in one
process, after a burn-in of random steps that leaves the envs in ordinary mid-episode states:
  us per call      `--calls` (50) back-to-back calls with out= given between two HIP events, device time per call with the launches
                   queued ahead (the kernel's own time plus the gap between two launches), for fingerprint(FP_DYNAMICS),
                   fingerprint(FP_VISIBLE) and fingerprint_parts(); `--rounds` rounds, alternated, every round kept
  bytes per env    what the kernel reads of an env for that part mask, from state_spec and the records: the mat row, 16 bytes per
                   slot of the live prefix (min(nobj, max_objects), the batch's mean), the mt row, the record, two bytes per seen chunk
  fraction of HBM  bytes per call / time per call over the 8.0 TB/s peak of the part (MI355X).  At 4096 envs the 35 MB a call reads
                   stay in the 256 MB last-level cache from one call to the next: that figure is a rate, not HBM traffic.
Every window ends in a device synchronise.
"""
import argparse
import json
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SEED, TAPE_SEED = 1000, 1234   # bench.py's convention
CONFIGS = (('4096', 4096, (64, 64)), ('8192x256x256', 8192, (256, 256)))
HBM_PEAK = 8.0e12   # bytes / s


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


def bytes_per_env(env, parts):
  """Bytes crafter_fingerprint reads of one env for the part mask `parts` (the batch's mean), from state_spec and the records."""
  from crafter_amd import abi, state
  spec = state.state_spec(env.cfg)
  row = lambda name: int(np.prod(spec[name][0][1:])) * np.dtype(spec[name][1]).itemsize
  rec = env.records()
  total = row('rec')
  if parts & abi.FP_MAP:
    total += row('mat')
  if parts & abi.FP_OBJECTS:
    total += abi.OBJ_DTYPE.itemsize * float(np.minimum(rec['nobj'], env.cfg.max_objects).mean())
  if parts & abi.FP_RNG:
    total += row('mt')
  if parts & abi.FP_CHUNKS:
    total += 2 * float(np.minimum(rec['nchunks_seen'], spec['chunk_order'][0][1]).mean())
  return total


def measure(envs, area, args):
  import torch
  from crafter_amd import BatchedEnv, abi
  env = BatchedEnv(envs, seed=SEED, area=area, auto_reset=True, render=False)
  env.reset()
  tape = torch.from_numpy(np.random.RandomState(TAPE_SEED).randint(0, 17, size=(args.burn_in, envs)).astype(np.int32)).cuda()
  env.rollout(tape, obs=False)
  env.check_errors()
  key = torch.zeros(envs, dtype=torch.int64, device='cuda')
  parts = torch.zeros((envs, abi.FP_PARTS), dtype=torch.int64, device='cuda')
  calls = {'dynamics': (abi.FP_DYNAMICS, lambda: env.fingerprint(abi.FP_DYNAMICS, out=key)),
           'visible': (abi.FP_VISIBLE, lambda: env.fingerprint(abi.FP_VISIBLE, out=key)),
           'parts': (abi.FP_ALL, lambda: env.fingerprint_parts(out=parts))}
  for _, fn in calls.values():
    per_call(fn, args.calls)
  us = {k: [] for k in calls}
  for _ in range(args.rounds):
    for k, (_, fn) in calls.items():
      us[k].append(per_call(fn, args.calls))
  med = lambda v: float(np.median(v))
  rec = env.records()
  res = {'envs': envs, 'area': list(area), 'slot_map_derived': bool(env.slot_map_derived), 'max_objects': int(env.cfg.max_objects),
         'mean_nobj': round(float(rec['nobj'].mean()), 1), 'distinct_keys': int(torch.unique(key).numel()), 'calls': {}}
  for k, (mask, _) in calls.items():
    b = bytes_per_env(env, mask)
    t = med(us[k]) * 1e-6
    res['calls'][k] = {'us_per_call': [round(x, 3) for x in us[k]], 'us_per_call_median': round(med(us[k]), 3),
                       'bytes_per_env': round(b, 1), 'mbytes_per_call': round(b * envs / 1e6, 2),
                       'tbytes_per_s': round(b * envs / t / 1e12, 3), 'fraction_of_hbm_peak': round(b * envs / t / HBM_PEAK, 4)}
  del env
  return res


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--configs', nargs='+', default=[c[0] for c in CONFIGS], choices=[c[0] for c in CONFIGS])
  ap.add_argument('--calls', type=int, default=50)
  ap.add_argument('--burn-in', type=int, default=64)
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--out', default=str(ROOT / 'profiles' / 'fingerprint.json'))
  args = ap.parse_args()
  import torch
  from crafter_amd.build import source_hash
  out = pathlib.Path(args.out)
  out.parent.mkdir(parents=True, exist_ok=True)
  doc = {'what': {'us_per_call': 'HIP events around `calls` back-to-back calls (out= given), device time per call',
                  'bytes_per_env': 'mat row + 16 B per slot of the live prefix + mt row + record + 2 B per seen chunk, for the part mask',
                  'fraction_of_hbm_peak': 'bytes per call / time per call / 8.0 TB/s; 4096 envs of the default geometry fit the last-level cache'},
         'calls': args.calls, 'burn_in': args.burn_in, 'rounds': args.rounds, 'seed': SEED, 'tape_seed': TAPE_SEED,
         'device': torch.cuda.get_device_name(0), 'results': {}, 'csrc_sha16': source_hash()}
  for name, envs, area in CONFIGS:
    if name in args.configs:
      doc['results'][name] = measure(envs, area, args)
      print(json.dumps({name: doc['results'][name]}), flush=True)
      out.write_text(json.dumps(doc, indent=1) + '\n')   # after every configuration: a run cut short keeps what it measured
  print(out)


if __name__ == '__main__':
  main()
