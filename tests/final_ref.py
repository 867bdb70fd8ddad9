"""TEST INFRASTRUCTURE: the workload the final-observation tests share (tests/test_final_host.py, tests/test_gpu_final_obs.py)
and what the oracle says about it.

Twenty-four envs, seeds 100 .. 123, length 190; env i plays np.random.RandomState(seed_i).randint(0, 17, size=200).  On these
tapes every first episode ends by step 198, by day and by night, awake and asleep, by death and at the time limit (CASES).

tests.rollout.oracle_rollouts(auto_reset=True) gives per step obs hash / reward / done and the terminal frames' hashes; finals()
adds what it does not keep of a terminal state: whether the player died (env.py:106-115, discount == 0), the symbolic pair
(tests/symbolic_ref.py) and what kind of frame it is."""
import functools

import numpy as np

from tests import rollout
from tests import symbolic_ref as sr
from tests.parity import sha8

SEEDS = tuple(range(100, 124))
LENGTH = 190
STEPS = 200
HOST_SEEDS = (111, 117, 101, 108, 104, 109)
# what the oracle found on these tapes when the tests were written; asserted again from its trajectory (assert_cases)
CASES = {
    'day deaths': (111, 117),
    'night deaths, awake': (101, 105, 112),
    'night deaths, asleep': (108, 116),
    'truncated at night': (104, 109, 113),
}


def tape(seed, steps=STEPS):
  return np.random.RandomState(seed).randint(0, 17, size=steps).astype(np.int32)


def _finals_of(args):
  seed, steps, kwargs = args
  from oracle.crafter_oracle import OracleEnv
  env = OracleEnv(seed=seed, **dict(kwargs))
  env.reset()
  out = []
  for t, a in enumerate(tape(seed, steps)):
    obs, _, done, info = env.step(int(a))
    if done:
      local, stats = sr.symbolic_of(env)
      out.append({'t': t, 'sha': sha8(obs), 'terminated': info['discount'] == 0, 'local': local, 'stats': stats,
                  'daylight': float(env.daylight), 'sleeping': bool(env.sleeping), 'step': int(env._step)})
      env.reset()
  return out


@functools.lru_cache(None)
def reference(seeds=SEEDS, steps=STEPS, kwargs=(('length', LENGTH),)):
  """-> (oracle_rollouts' dicts, finals: per env the list of its terminal states in order), computed once per argument set.
  Neither is modified by a test."""
  specs = [{'kwargs': dict(kwargs, seed=s), 'actions': tape(s, steps), 'auto_reset': True} for s in seeds]
  runs = rollout.oracle_rollouts(specs)
  import multiprocessing as mp
  import os
  workers = min(len(seeds), max(1, len(os.sched_getaffinity(0))))
  jobs = [(s, steps, kwargs) for s in seeds]
  if workers <= 1:
    fin = [_finals_of(j) for j in jobs]
  else:
    with mp.get_context('fork').Pool(workers, initializer=rollout._worker_init) as pool:
      fin = pool.map_async(_finals_of, jobs, chunksize=1).get(timeout=600)
  for run, f in zip(runs, fin):   # the two replays of one tape agree on the terminal frames
    assert [(x['t'], x['sha']) for x in f] == list(run.get('terminal_sha', []))
  return runs, fin


def assert_cases(seeds, fin):
  """The kinds of terminal frame the workload is there for occurred (first episodes), from the oracle's own trajectory."""
  first = {s: f[0] for s, f in zip(seeds, fin) if f}
  assert len(first) == len(seeds), 'an env never finished'
  day = [s for s, f in first.items() if f['terminated'] and f['daylight'] >= 0.5]
  night = [s for s, f in first.items() if f['terminated'] and f['daylight'] < 0.5]
  asleep = [s for s, f in first.items() if f['terminated'] and f['sleeping']]
  trunc = [s for s, f in first.items() if not f['terminated']]
  assert all(first[s]['step'] == LENGTH and first[s]['daylight'] < 0.5 for s in trunc)
  assert len(day) >= 2 and len(night) >= 2 and len(asleep) >= 1 and len(trunc) >= 2, (day, night, asleep, trunc)
  return {'day': day, 'night': night, 'asleep': asleep, 'truncated': trunc}
