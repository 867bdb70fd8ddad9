#!/usr/bin/env python3
"""What BatchedEnv.step(final=True) costs, on one GPU.  Not bench.py.

Three closed loops at 4096 envs with uniform random actions, `--steps` steps between synchronisations, `--repeats` windows
each, timed with HIP events around the window:
  A  step()                                           auto_reset=True: the loop every README number is measured on
  B  step(final=True)                                 the same, plus the finished episodes' last observation
  C  step(); reset(mask=done)  with auto_reset=False  the only way to that frame before crafter_step_final existed
A and C also run on a second library (--other NAME=PATH, e.g. a build of the parent commit: tools/ab_make.sh parent HEAD),
loaded through CRAFTER_HIP_LIB.  Every (library, loop) pair runs in a fresh child process -- a process loads one library --
and the pairs alternate over the repeats, so that drift of the box hits all of them alike.

  python tools/final_obs_cost.py --other parent=ab_builds/parent.so --out profiles/final_obs_cost.txt

Loop B also reports, from a window of its own with crafter_set_timing on, the share of the kernels' time that the second
kernel (crafter_requeue_final_kernel) takes, and the average number of envs it is handed per step."""
import argparse
import json
import os
import pathlib
import subprocess
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SEED, TAPE_SEED = 1000, 1234   # bench.py's convention


def child(args):
  import torch
  from crafter_amd import BatchedEnv
  loop, n = args.child, args.envs
  env = BatchedEnv(n, seed=SEED, auto_reset=loop != 'C')
  tape = torch.from_numpy(np.random.RandomState(TAPE_SEED).randint(0, 17, size=(512, n)).astype(np.int32)).cuda()

  def run(t0, steps):
    for t in range(t0, t0 + steps):
      a = tape[t % tape.shape[0]]
      if loop == 'A':
        env.step(a, info=False)
      elif loop == 'B':
        env.step(a, info=False, final=True)
      else:
        _, _, done, _ = env.step(a, info=False)
        env.reset(mask=done)
    return t0 + steps

  env.reset()
  pos = run(0, args.burn_in)
  torch.cuda.synchronize()
  rates = []
  for _ in range(args.repeats):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    pos = run(pos, args.steps)
    stop.record()
    stop.synchronize()
    rates.append(args.steps * n / (start.elapsed_time(stop) * 1e-3))
  out = {'loop': loop, 'env_steps_per_s': [round(r) for r in rates]}
  if loop == 'B':   # the second kernel's share and its queue, in a window of their own (timing mode attaches events to every launch)
    steps = min(args.steps, 500)
    env.set_timing(True)
    finished = torch.zeros((), dtype=torch.int64, device='cuda')
    for t in range(pos, pos + steps):
      _, _, done, _ = env.step(tape[t % tape.shape[0]], info=False, final=True)
      finished += done.sum()
    step_ms, second_ms, launches = env.get_timing()
    env.set_timing(False)
    out.update(step_kernel_ms=round(step_ms, 3), second_kernel_ms=round(second_ms, 3), launches=launches,
               second_kernel_share=round(second_ms / (step_ms + second_ms), 4), queued_per_step=round(int(finished) / steps, 2))
  env.check_errors()
  print('RESULT ' + json.dumps(out), flush=True)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--envs', type=int, default=4096)
  ap.add_argument('--steps', type=int, default=2000)
  ap.add_argument('--burn-in', type=int, default=400)
  ap.add_argument('--repeats', type=int, default=3)
  ap.add_argument('--other', default='', help='NAME=PATH of a second library for loops A and C')
  ap.add_argument('--out', default='')
  ap.add_argument('--child', default='', choices=('', 'A', 'B', 'C'))
  args = ap.parse_args()
  if args.child:
    return child(args)
  libs = {'tree': ''}
  if args.other:
    name, path = args.other.split('=', 1)
    libs[name] = str(pathlib.Path(path).resolve())
  pairs = [(lib, loop) for loop in 'ABC' for lib in libs if not (loop == 'B' and lib != 'tree')]
  res = {p: {'env_steps_per_s': []} for p in pairs}
  for _ in range(args.repeats):   # one window per pair and round, the pairs alternating
    for lib, loop in pairs:
      env = dict(os.environ)
      env.pop('CRAFTER_HIP_LIB', None)
      if libs[lib]:
        env['CRAFTER_HIP_LIB'] = libs[lib]
      cmd = [sys.executable, __file__, '--child', loop, '--envs', str(args.envs), '--steps', str(args.steps), '--burn-in', str(args.burn_in),
             '--repeats', '1']
      proc = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
      if proc.returncode != 0:
        raise SystemExit(f'{lib} {loop}: exit {proc.returncode}\n{proc.stderr[-3000:]}')
      got = json.loads([l for l in proc.stdout.splitlines() if l.startswith('RESULT ')][-1][7:])
      res[(lib, loop)]['env_steps_per_s'] += got.pop('env_steps_per_s')
      got.pop('loop')
      res[(lib, loop)].update(got)
      print(lib, loop, res[(lib, loop)], flush=True)
  import torch
  lines = [f'final_obs_cost: {args.envs} envs, {args.steps} steps per window, {args.repeats} windows per loop (one per child process, alternating), '
           f'burn-in {args.burn_in}, HIP events; {torch.cuda.get_device_name(0) if torch.cuda.is_available() else "no device"}']
  for (lib, loop), r in res.items():
    v = r['env_steps_per_s']
    extra = {k: x for k, x in r.items() if k != 'env_steps_per_s'}
    lines.append(f'{loop} {lib:8s} median {np.median(v) / 1e6:7.3f} M env-steps/s  min {min(v) / 1e6:7.3f}  max {max(v) / 1e6:7.3f}  '
                 f'us/step {1e6 * args.envs / np.median(v):7.2f}' + (f'  {json.dumps(extra)}' if extra else ''))
  text = '\n'.join(lines) + '\n'
  print(text)
  if args.out:
    pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(args.out).write_text(text)


if __name__ == '__main__':
  main()
