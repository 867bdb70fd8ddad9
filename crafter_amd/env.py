"""``crafter_amd.Env`` -- drop-in for the reference ``crafter.Env`` (env.py:25-133) on one MI355X.

Same constructor, same ``reset() -> obs``, ``step(a) -> (obs, reward, done, info)``,
``render(size=None)``, ``observation_space`` / ``action_space`` / ``action_names``, the same
old-gym conventions (no auto-reset, obs only from reset) and the private attributes in-repo
callers touch (``_step``, ``_world.count``, ``_player.achievements/.sleeping``; run_random.py:32-42,
run_gui.py:70,105-122).  It is ``BatchedEnv(1)`` plus host copies: every call synchronises, so use
``BatchedEnv`` for throughput.
"""
import collections

import numpy as np
import torch

from . import abi, batched, tables, worlds as _worlds

try:  # gym is optional in the reference too (env.py:11-22)
  import gym
  DiscreteSpace = gym.spaces.Discrete
  BoxSpace = gym.spaces.Box
  BaseClass = gym.Env
except ImportError:
  DiscreteSpace = collections.namedtuple('DiscreteSpace', 'n')
  BoxSpace = collections.namedtuple('BoxSpace', 'low, high, shape, dtype')
  BaseClass = object


class _WorldView:
  """What callers read through ``env._world`` (run_random.py:32-34, run_terrain.py:23)."""

  def __init__(self, env):
    self._env = env
    self.area = env._area

  def count(self, material):
    ids = {name: i + 1 for i, name in enumerate(self._env._batch.rules['materials'])}
    mat = self._env._batch.state['mat'][0]
    return int((mat == ids[material]).sum().item())

  @property
  def daylight(self):
    return float(self._env._batch.tables.daylight[self._env._step or 0])


class _PlayerView:
  """What callers read through ``env._player`` (run_gui.py:105,116; recorder via info)."""

  def __init__(self, env):
    self._env = env

  def _rec(self):
    return self._env._batch.records()[0]

  @property
  def inventory(self):
    r = self._rec()
    return {n: int(r['inv'][i]) for i, n in enumerate(self._env._batch.item_names)}

  @property
  def achievements(self):
    r = self._rec()
    return {n: int(r['ach'][i]) for i, n in enumerate(self._env._batch.achievement_names)}

  @property
  def sleeping(self):
    return bool(self._rec()['sleeping'])

  @property
  def health(self):
    return self.inventory['health']

  @property
  def pos(self):
    return self._env._batch.info()['player_pos'][0].cpu().numpy().astype(np.int64)


class Env(BaseClass):

  def __init__(self, area=(64, 64), view=(9, 9), size=(64, 64), reward=True, length=10000, seed=None,
               device='cuda', rules=None):
    view = np.array(view if hasattr(view, '__len__') else (view, view))
    size = np.array(size if hasattr(size, '__len__') else (size, size))
    seed = np.random.randint(0, 2 ** 31 - 1) if seed is None else seed  # env.py:32
    self._area = area
    self._view = view
    self._size = size
    self._reward = reward
    self._length = length
    self._seed = seed
    self._episode = 0
    self._rules = rules
    self._batch = batched.BatchedEnv(
        1, area, tuple(int(v) for v in view), tuple(int(s) for s in size), reward, length, seeds=[seed],
        device=device, auto_reset=False, semantic=True, render=True, rules=rules)
    self._world = _WorldView(self)
    self._player = None
    self._step = None
    self.reward_range = None
    self.metadata = None

  # copy.deepcopy / pickle (the reference's Env is a plain Python object: both carry the whole world, the RNG, _seed and
  # _episode).  The copy is a new Env -- its own native handle -- whose device row is loaded from the original's.
  def _ctor_args(self):
    return dict(area=self._area, view=tuple(int(v) for v in self._view), size=tuple(int(v) for v in self._size), reward=self._reward,
                length=self._length, seed=self._seed, rules=self._rules)

  def _restore(self, host, store, device):
    Env.__init__(self, device=device, **host['ctor'])
    self._episode, self._step = host['episode'], host['step']
    self._player = _PlayerView(self) if host['player'] else None
    self._batch.load_state(store.to(self._batch.device), [0], [0])

  def _host_fields(self):
    return {'ctor': self._ctor_args(), 'episode': self._episode, 'step': self._step, 'player': self._player is not None}

  def __deepcopy__(self, memo):
    new = Env.__new__(Env)
    memo[id(self)] = new
    new._restore(self._host_fields(), self._batch.save_state([0]), self._batch.device)
    return new

  def __getstate__(self):
    return {'host': self._host_fields(), 'store': self._batch.save_state([0]).cpu()}

  def __setstate__(self, state):
    self._restore(state['host'], state['store'], 'cuda')

  @property
  def observation_space(self):
    return BoxSpace(0, 255, tuple(self._size) + (3,), np.uint8)

  @property
  def action_space(self):
    return DiscreteSpace(len(self._batch.action_names))

  @property
  def action_names(self):
    return self._batch.action_names

  def reset(self, seed=None, episode=None, world=None):
    """Env.reset() (env.py:70-81).  seed (Gymnasium's reset(seed=...)): the env becomes crafter.Env(seed=seed) at its
    episode-th reset (default 1) -- that level, and the episodes that follow it; _seed and _episode say so, and a deepcopy
    or pickle taken afterwards carries the new seed.  episode alone restarts the current seed at that episode.
    world: dict(mat [W, H], objects, inventory=None) -- one world in the form of crafter_amd.WorldBank (what export_world()
    returns): this episode plays in it instead of a generated world; the next reset() generates again."""
    bank = None
    if world is not None:   # (raises ValueError before anything changes)
      inv = world.get('inventory')
      bank = _worlds.WorldBank(self._batch, np.asarray(world['mat'])[None], [world.get('objects', [])], None if inv is None else [inv])
    if seed is None and episode is None:
      self._episode += 1
      self._step = 0
      obs = self._batch.reset(worlds=bank)
    else:
      episode = 1 if episode is None else int(episode)
      obs = self._batch.reset(seeds=None if seed is None else [seed], episodes=[episode], worlds=bank)   # (raises before anything changes)
      if seed is not None:
        self._seed = seed
      self._episode = episode
      self._step = 0
    self._player = _PlayerView(self)
    out = obs[0].cpu().numpy()
    self._batch.check_errors()
    return out

  def step(self, action):
    b = self._batch
    action = int(action)
    if not 0 <= action < len(b.action_names):
      # the reference indexes a Python list (env.py:86); negative indices are rejected here too
      raise IndexError('list index out of range')
    self._step += 1
    acts = torch.tensor([action], dtype=torch.int32, device=b.device)
    obs, _, _, _ = b.step(acts, info=False)
    obs = obs[0].cpu().numpy()
    b.check_errors()
    r = b.records()[0]
    reward = int(r['dhealth']) / 10              # env.py:97
    if int(r['new_unlocked']):
      reward += 1.0                              # env.py:102-104
    dead = bool(r['dead'])
    over = self._length and self._step >= self._length
    done = dead or over
    info = {
        'inventory': {n: int(r['inv'][i]) for i, n in enumerate(b.item_names)},
        'achievements': {n: int(r['ach'][i]) for i, n in enumerate(b.achievement_names)},
        'discount': 1 - float(dead),
        'semantic': b.state['semantic'][0].cpu().numpy().reshape(b.cfg.W, b.cfg.H),
        'player_pos': self._player.pos,
        'reward': reward,
    }
    if not self._reward:
      reward = 0.0
    return obs, reward, done, info

  def export_world(self):
    """The world as it stands, in the form reset(world=...) takes: dict(mat [W, H], objects, inventory)."""
    w = self._batch.export_worlds([0])
    return dict(mat=w['mat'][0], objects=w['objects'][0], inventory=w['inventory'][0])

  def edit(self, ops):
    """BatchedEnv.edit for this env: ops is one tape of crafter_amd.edits ops (set_cell, add, remove, move, set_object,
    set_item, set_player, set_clock), applied in order to the episode under way -- `env._world[x, y] = ...`,
    `env._world.add(...)`, `env._player.inventory[...] = ...` of the reference.  render() shows the result at once; an op the
    device had to refuse raises CrafterDeviceError (ST_BAD_EDIT) with the tape's other ops applied."""
    self._batch.edit([0], list(ops))
    try:
      self._batch.check_errors()
    finally:   # (a clock op moves it -- also in a tape with a refused op: the other ops were applied)
      self._step = int(self._batch.records()[0]['step'])

  def render(self, size=None):
    size = None if size is None else tuple(int(v) for v in (size if hasattr(size, '__len__') else (size, size)))
    return self._batch.render(size)[0].cpu().numpy()

  def symbolic(self):
    """BatchedEnv.symbolic() for this env: (local uint8 [2, gw, gh], stats float32 [n_items + 4]) as numpy arrays."""
    local, stats = self._batch.symbolic()
    return local[0].cpu().numpy(), stats[0].cpu().numpy()

  def set_levels(self, seeds, episodes=None, weights=None, key=0):
    """BatchedEnv.set_levels for this env: its coming reset()s draw their level from the table (None: clear).
    The table belongs to this object's native handle: a deepcopy or pickle carries seed and episode count, not the table -- set
    it on the copy."""
    return self._batch.set_levels(seeds, episodes, weights, key)

  def legal_actions(self):
    """BatchedEnv.legal_actions() for this env: bool [n_actions], True where the action passes its guards in the current state."""
    return self._batch.legal_actions()[0].cpu().numpy().astype(bool)

  def navigate(self, targets, passable=None):
    """BatchedEnv.navigate(targets, passable) for this env: (dist int32 [K], first int32 [K], facing bool [K]) as numpy arrays."""
    dist, first, facing = self._batch.navigate(targets, passable)
    return dist[0].cpu().numpy(), first[0].cpu().numpy(), facing[0].cpu().numpy().astype(bool)

  def nearby(self, distance=None, k=16, classes=None, numpy_slices=False):
    """BatchedEnv.nearby(...) for this env: (counts int32 [C], ents int16 [k, 6], n) as numpy arrays and an int, plus the counts
    as a {class name: count} dict ('none': the cells of the window) -- World.nearby and World.count of the reference in one call."""
    counts, ents, n = self._batch.nearby(distance, k, classes, numpy_slices)
    counts = counts[0].cpu().numpy()
    return counts, ents[0].cpu().numpy(), int(n[0].item()), dict(zip(self._batch.symbolic_names['classes'], counts.tolist()))

  def audit(self):
    """BatchedEnv.audit() for this env: the names (abi.AUDIT_NAMES) of the invariants its row fails; [] for a consistent one."""
    bits = int(self._batch.audit()[0][0].item())
    return [name for b, name in enumerate(abi.AUDIT_NAMES) if bits >> b & 1]

  def fingerprint(self, parts=abi.FP_DYNAMICS):
    """BatchedEnv.fingerprint(parts) for this env: the key as an unsigned Python int."""
    return int(self._batch.fingerprint(parts)[0].item()) & 0xFFFFFFFFFFFFFFFF
