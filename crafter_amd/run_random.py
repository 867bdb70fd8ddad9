"""``python -m crafter_amd.run_random`` -- the reference's ``crafter/run_random.py`` (lines 10-44) on the
MI355X path: same flags, same prints (reset time, material counts, step time / FPS, episode length).
``--envs N`` (not in the reference) runs N environments at once through BatchedEnv; ``--legal`` (not in the reference either)
samples uniformly among the actions the legal-action mask allows instead of among all of them; ``--levels K`` (not in the
reference) draws every episode from a level table of seeds 0 .. K-1 (BatchedEnv.set_levels); ``--worlds FILE.npz`` (not in the
reference) plays the authored worlds of a bank saved by ``WorldBank.save`` instead of generated ones; ``--audit K`` (not in the
reference) audits every row after every K-th step (BatchedEnv.assert_consistent) and stops with the finding; ``--census`` (not in
the reference) prints the reference's three "exist" lines for every env after the reset, from one BatchedEnv.nearby call."""
import argparse
import copy
import time

import numpy as np


def sample_legal(legal, generator=None):
  """One action per row of the mask `legal` (uint8 / bool [N, n_actions] tensor), uniform among the row's non-zero entries
  (noop is always one) -> int32 [N] on the mask's device."""
  import torch
  return torch.multinomial(legal.to(torch.float32), 1, generator=generator).reshape(-1).to(torch.int32)


def main(argv=None):
  parser = argparse.ArgumentParser()
  parser.add_argument('--seed', type=int, default=None)
  parser.add_argument('--area', nargs=2, type=int, default=(64, 64))
  parser.add_argument('--length', type=int, default=10000)
  parser.add_argument('--health', type=int, default=9)
  parser.add_argument('--record', type=str, default=None)
  parser.add_argument('--episodes', type=int, default=1)
  parser.add_argument('--envs', type=int, default=1)
  parser.add_argument('--legal', action='store_true', help='sample uniformly among the legal actions (BatchedEnv.legal_actions)')
  parser.add_argument('--levels', type=int, default=0, help='draw every episode from a level table of seeds 0 .. K-1 (set_levels)')
  parser.add_argument('--worlds', type=str, default=None, help='play the authored worlds of a bank saved by WorldBank.save (reset(worlds=...))')
  parser.add_argument('--audit', type=int, default=0, help='audit every row after every K-th step and stop with the finding (assert_consistent)')
  parser.add_argument('--census', action='store_true', help='print the three "exist" lines for every env after the reset, from one nearby() call')
  args = parser.parse_args(argv)

  import torch
  from . import BatchedEnv, Env, tables
  from .recorder import BatchedStatsRecorder, EnvStatsRecorder
  rules = copy.deepcopy(tables.load_rules())
  rules['items']['health']['max'] = args.health       # run_random.py:21-22
  rules['items']['health']['initial'] = args.health
  random = np.random.RandomState(args.seed)

  def audit(batch, step):   # --audit K: raises CrafterDeviceError naming the rows, the invariants they fail and where
    if args.audit > 0 and step % args.audit == 0:
      batch.assert_consistent()

  def census(batch):   # --census: World.count of coal, iron and diamond for every env, one launch and one download
    if not args.census:
      return
    names = batch.symbolic_names['classes']
    counts = batch.nearby(None, k=0)[0].cpu().numpy()
    for e, row in enumerate(counts):
      print(f'Env {e}:')
      print('Coal exist:    ', int(row[names.index('coal')]))
      print('Iron exist:    ', int(row[names.index('iron')]))
      print('Diamonds exist:', int(row[names.index('diamond')]))

  def legal_generator(device):   # --legal: torch.multinomial's stream, on the device the mask lives on
    generator = torch.Generator(device=device)
    generator.manual_seed(0 if args.seed is None else args.seed)
    return generator

  if args.worlds:   # authored worlds: every episode of every env plays a world of the bank, chosen at random on the device
    from . import WorldBank
    bank = WorldBank.load(args.worlds, rules)
    seed = 0 if args.seed is None else args.seed
    env = BatchedEnv(args.envs, area=bank.area, length=args.length, seed=seed, rules=rules, auto_reset=False)
    generator = torch.Generator(device=env.device)
    generator.manual_seed(seed)
    pick = lambda: torch.randint(0, len(bank), (args.envs,), generator=generator, device=env.device, dtype=torch.int32)
    legal = legal_generator(env.device) if args.legal else None
    start = time.time()
    env.reset(worlds=bank, world_ids=pick())
    torch.cuda.synchronize()
    print(f'Reset time: {1000 * (time.time() - start):.2f}ms for {args.envs} envs into {len(bank)} authored worlds')
    census(env)
    finished, steps = 0, 0
    start = time.time()
    while finished < args.episodes * args.envs:
      if args.legal:
        actions = sample_legal(env.legal_actions(), legal)
      else:
        actions = torch.from_numpy(random.randint(0, env.num_actions, size=args.envs).astype(np.int32)).to(env.device)
      _, _, done, _ = env.step(actions, info=False)
      env.reset(mask=done, worlds=bank, world_ids=pick())   # no host round trip: the mask stays on the device
      steps += args.envs
      audit(env, steps // args.envs)
      if steps // args.envs % 64 == 0:
        finished = int(env.records()['episode'].sum()) - args.envs
    torch.cuda.synchronize()
    duration = time.time() - start
    env.check_errors()
    print(f'Step time: {1000 * duration / (steps / args.envs):.3f}ms per batched step ({int(steps / duration)} env-steps/s)')
    print('Episodes finished:', int(env.records()['episode'].sum()) - args.envs)
    return

  if args.envs == 1:
    env = Env(area=tuple(args.area), length=args.length, seed=args.seed, rules=rules)
    batch = env._batch
    if args.record:   # run_random.py:24: crafter.Recorder(env, args.record) -> stats.jsonl
      env = EnvStatsRecorder(env, args.record)
    if args.levels:
      env.set_levels(list(range(args.levels)))
    generator = legal_generator('cpu') if args.legal else None
    for _ in range(args.episodes):
      start = time.time()
      env.reset()
      print('')
      print(f'Reset time: {1000 * (time.time() - start):.2f}ms')
      print('Coal exist:    ', env._world.count('coal'))
      print('Iron exist:    ', env._world.count('iron'))
      print('Diamonds exist:', env._world.count('diamond'))
      census(batch)
      start = time.time()
      done = False
      while not done:
        if args.legal:
          action = int(sample_legal(torch.from_numpy(env.legal_actions()[None]), generator)[0])
        else:
          action = random.randint(0, env.action_space.n)
        _, _, done, _ = env.step(action)
        audit(batch, env._step)
      duration = time.time() - start
      step = env._step
      print(f'Step time: {1000 * duration / step:.2f}ms ({int(step / duration)} FPS)')
      print('Episode length:', step)
    return

  seed = 0 if args.seed is None else args.seed
  env = batch = BatchedEnv(args.envs, area=tuple(args.area), length=args.length, seed=seed, rules=rules, auto_reset=True)
  if args.levels:
    env.set_levels(list(range(args.levels)))
  if args.record:
    env = BatchedStatsRecorder(env, args.record)
  generator = legal_generator(env.device) if args.legal else None
  start = time.time()
  env.reset()
  torch.cuda.synchronize()
  print(f'Reset time: {1000 * (time.time() - start):.2f}ms for {args.envs} envs')
  census(batch)
  finished, steps = 0, 0
  start = time.time()
  while finished < args.episodes * args.envs:
    if args.legal:
      actions = sample_legal(env.legal_actions(), generator)
    else:
      actions = torch.from_numpy(random.randint(0, env.num_actions, size=args.envs).astype(np.int32)).to(env.device)
    _, _, done, _ = env.step(actions, info=False)
    finished += int(done.sum())
    steps += args.envs
    audit(batch, steps // args.envs)
  torch.cuda.synchronize()
  duration = time.time() - start
  env.check_errors()
  print(f'Step time: {1000 * duration / (steps / args.envs):.3f}ms per batched step ({int(steps / duration)} env-steps/s)')
  print('Episodes finished:', finished)


if __name__ == '__main__':
  main()
