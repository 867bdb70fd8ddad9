"""The runs of tests/test_oracle_vs_reference.py as digests: one side of the comparison can be stored and the other
checked against it later.

tools/make_reference_runs.py plays every run on the UNTOUCHED reference (oracle/reference_harness.py) and stores its
digests in tests/golden/reference_runs/oracle_vs_reference.npz; the test plays the same runs on the oracle and compares.  Every value
that the test compared between the two envs enters a digest here.  Values are normalised first, so that values that
compare equal digest alike (an int and an np.int64, a uint8 and an int64 array)."""
import hashlib

import numpy as np

from tests import scenarios

FIXTURE = 'reference_runs/oracle_vs_reference.npz'
# a run is a list of rows (kind, four digests); what the digests of each kind cover, for the messages of the test
KINDS = {0: ('reset obs', 'material map', '-', 'objects'),
         1: ('obs', 'reward / done / info', 'semantic view', 'objects / chunk order / RNG'),
         2: ('render()', '-', '-', '-')}


def digest(*parts):
  h = hashlib.sha256()
  for p in parts:
    if isinstance(p, np.ndarray):
      assert p.dtype.kind in 'biu', p.dtype
      h.update(repr(p.shape).encode() + np.ascontiguousarray(p, np.int64).tobytes())
    else:
      h.update(repr(p).encode())
    h.update(b'\0')
  return int.from_bytes(h.digest()[:8], 'little')


class ReferenceSide:
  """The state a reference ``crafter.Env`` exposes (tools/make_reference_runs.py only: it needs the reference tree)."""

  def __init__(self, env):
    self.env = env

  def give(self, item, amount):
    self.env._player.inventory[item] = amount

  def mat(self):
    return self.env._world._mat_map

  def objects(self):
    from crafter import objects as robj
    types = {robj.Player: 1, robj.Cow: 2, robj.Zombie: 3, robj.Skeleton: 4, robj.Arrow: 5, robj.Plant: 6}
    out = []
    for o in self.env._world._objects:
      if o is None:
        continue
      t = types[type(o)]
      f = tuple(int(v) for v in getattr(o, 'facing', (0, 0)))
      aux = {3: getattr(o, 'cooldown', 0), 4: getattr(o, 'reload', 0), 6: getattr(o, 'grown', 0)}.get(t, 0)
      out.append((t, int(o.pos[0]), int(o.pos[1]), int(o.health), f[0], f[1], int(aux)))
    return out

  def chunk_order(self):
    return list(self.env._world._chunks.keys())

  def rng(self):
    return self.env._world.random.get_state()


class OracleSide:
  """The same state of an ``OracleEnv``."""

  def __init__(self, env):
    self.env = env

  def give(self, item, amount):
    self.env.inv[self.env.t.item_id[item]] = amount

  def mat(self):
    return self.env.mat

  def objects(self):
    return self.env.objects()

  def chunk_order(self):
    return self.env.chunk_order

  def rng(self):
    return self.env.random.get_state()


def objects_digest(side):
  return digest([tuple(int(v) for v in o) for o in side.objects()])


def reset_row(side, obs):
  return (0, digest(np.asarray(obs)), digest(np.asarray(side.mat())), 0, objects_digest(side))


def step_row(side, result):
  obs, reward, done, info = result
  outcome = digest(type(reward).__name__, float(reward), bool(done),   # done None (length=None) counts as False
                   sorted((k, int(v)) for k, v in info['inventory'].items()),
                   sorted((k, int(v)) for k, v in info['achievements'].items()),
                   float(info['discount']), float(info['reward']), np.asarray(info['player_pos']))
  _, key, pos = side.rng()[:3]
  world = digest([tuple(int(v) for v in o) for o in side.objects()], [tuple(int(v) for v in k) for k in side.chunk_order()],
                 int(pos), np.asarray(key))
  return (1, digest(np.asarray(obs)), outcome, digest(np.asarray(info['semantic'])), world)


def play(make, seed, steps, tape=None, gifts=None, episodes=1, **kw):
  """make(seed=..., **kw) -> (env, side).  Resets `episodes` times; steps until done or `steps` steps, with actions from
  `tape` or RandomState(seed + 99); gifts[t] = {item: amount} written into the inventory before step t."""
  env, side = make(seed=seed, **kw)
  rs = np.random.RandomState(seed + 99)
  rows = []
  for _ in range(episodes):
    rows.append(reset_row(side, env.reset()))
    for t in range(steps):
      if gifts and t in gifts:
        for item, amount in gifts[t].items():
          side.give(item, amount)
      a = int(tape[t]) if tape is not None else int(rs.randint(0, 17))
      result = env.step(a)
      rows.append(step_row(side, result))
      if result[2]:
        break
  return rows


def play_night_renders(make):
  """Extra render() calls at night: each draws 3087 doubles of night noise (engine.py:209) from the world's RNG."""
  env, side = make(seed=7)
  rows = [reset_row(side, env.reset())]
  for t in range(200):
    result = env.step(0 if t % 3 else 6)
    if t > 150 and t % 7 == 0:
      rows.append((2, digest(np.asarray(env.render())), 0, 0, 0))
    rows.append(step_row(side, result))
    if result[2]:
      break
  return rows


def scripted(kind):
  acts, gifts = scenarios.SCENARIOS[kind](300, 5)
  return lambda make: play(make, 5, 300, tape=acts, gifts=gifts)


RUNS = {
    **{f'random_s{seed}': (lambda make, seed=seed: play(make, seed, 350, episodes=2)) for seed in range(4)},
    **{f'scripted_{kind}': scripted(kind) for kind in sorted(scenarios.SCENARIOS)},
    'variant_area_view_size': lambda make: play(make, 4, 80, area=(32, 48), view=(7, 9), size=(84, 84)),   # other view / unit 12 x 9 / border
    'variant_length_no_reward': lambda make: play(make, 6, 60, length=40, reward=False),                  # `over` + zeroed reward
    'variant_unbounded_length': lambda make: play(make, 8, 60, length=None),                              # done is None-ish until death
    'night_renders': play_night_renders,
}


def worlds(make, seed, episodes):
  """(material map, objects digest) after each of `episodes` consecutive reset() calls."""
  env, side = make(seed=seed)
  out = []
  for _ in range(episodes):
    env.reset()
    out.append((np.array(side.mat(), copy=True), objects_digest(side)))
  return out
