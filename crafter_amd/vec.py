"""A vector-env view of ``BatchedEnv`` with the method surface Stable-Baselines3's ``VecEnv`` and similar
trainers expect (numpy in / numpy out, ``step_async`` + ``step_wait``, auto-reset with
``infos[i]['terminal_observation']``), SURVEY.md section 8f row 3.

No dependency on SB3 / gymnasium (neither is required by the reference, and neither is in this image): the
class only follows the protocol, so it can be handed to anything that duck-types a VecEnv.

The finished episode's last frame has to be reported.  By default the wrapped env runs with ``auto_reset=False``
and finished envs are reset here with one masked ``reset`` (the in-kernel auto-reset of ``BatchedEnv``
draws the next episode's first frame over it).  ``info`` follows the reference (env.py:108-115):
inventory / achievements dicts, discount, player_pos, reward (+ semantic when asked for).

``VecEnvView(..., auto_reset=True)`` keeps the in-kernel auto-reset (world pool included) and takes the last frame from
``BatchedEnv.step(final=True)`` instead: ``terminal_observation`` is ``final_obs``, ``TimeLimit.truncated`` is
``terminated == 0``, and there is no masked ``reset``.  obs / reward / done and those two are identical to the default mode.
The host-side info of an env that finished is then put together from what the finished episode left behind: inventory from
``final_stats``, achievements from the ``terminal`` row, discount from ``terminated``, reward from the step's reward (with
``reward=False`` the batch returns 0 and so does this entry).  Not reproduced for such an env: ``player_pos`` and
``semantic`` describe the new episode's first state.
"""
import numpy as np
import torch

from .batched import BatchedEnv
from .env import BoxSpace, DiscreteSpace


class VecEnvView:

  def __init__(self, num_envs, area=(64, 64), view=(9, 9), size=(64, 64), reward=True, length=10000, seed=None,
               seeds=None, device='cuda', semantic=False, auto_reset=False, **kwargs):
    self._auto_reset = bool(auto_reset)
    self._batch = BatchedEnv(num_envs, area=area, view=view, size=size, reward=reward, length=length, seed=seed,
                             seeds=seeds, device=device, auto_reset=self._auto_reset, semantic=semantic, **kwargs)
    self.num_envs = int(num_envs)
    b = self._batch
    self.observation_space = BoxSpace(0, 255, tuple(b.observation_shape), np.uint8)
    self.action_space = DiscreteSpace(b.num_actions)
    self.action_names = list(b.action_names)
    self.reward_range = None
    self.metadata = None
    self._semantic = bool(semantic)
    self._length = length
    self._pending = None

  @property
  def batch(self):
    """The underlying ``BatchedEnv`` (device tensors)."""
    return self._batch

  # ------------------------------------------------------------------ VecEnv protocol
  def reset(self):
    return self._batch.reset().cpu().numpy()

  def step_async(self, actions):
    self._pending = torch.as_tensor(np.asarray(actions), dtype=torch.int32).to(self._batch.device)

  def step_wait(self):
    b = self._batch
    obs, reward, done, info = b.step(self._pending, final=self._auto_reset)
    self._pending = None
    b.check_errors()
    rec = b.records()
    obs_h, rew_h = obs.cpu().numpy().copy(), reward.cpu().numpy().copy()
    done_h = done.cpu().numpy().astype(bool)
    if self._auto_reset and done_h.any():   # what the finished episodes left behind (rows valid where done)
      final_obs = info['final_obs'].cpu().numpy() if 'final_obs' in info else np.zeros_like(obs_h)
      terminated = info['terminated'].cpu().numpy().astype(bool)
      final_stats = info['final_stats'].cpu().numpy()
      terminal = b.terminal.cpu().numpy()
    pos = info['player_pos'].cpu().numpy().astype(np.int64)
    sem = info['semantic'].cpu().numpy() if self._semantic else None
    infos = []
    for i in range(self.num_envs):
      r = rec[i]
      dead = bool(r['dead'])
      d = {
          'inventory': {n: int(r['inv'][k]) for k, n in enumerate(b.item_names)},
          'achievements': {n: int(r['ach'][k]) for k, n in enumerate(b.achievement_names)},
          'discount': 1 - float(dead),
          'player_pos': pos[i],
          'reward': int(r['dhealth']) / 10 + (1.0 if int(r['new_unlocked']) else 0.0),
      }
      if sem is not None:
        d['semantic'] = sem[i].copy()
      if done_h[i] and self._auto_reset:   # `rec` is the new episode's already
        dead = bool(terminated[i])
        d['inventory'] = {n: int(final_stats[i, k]) for k, n in enumerate(b.item_names)}
        d['achievements'] = {n: int(terminal[i, k]) for k, n in enumerate(b.achievement_names)}
        d['discount'] = 1 - float(dead)
        d['reward'] = float(rew_h[i])
        d['terminal_observation'] = final_obs[i].copy()
        d['TimeLimit.truncated'] = not dead
      elif done_h[i]:
        d['terminal_observation'] = obs_h[i].copy()
        d['TimeLimit.truncated'] = not dead   # the episode ran into `length` (env.py:106-107)
      infos.append(d)
    if done_h.any() and not self._auto_reset:
      fresh = b.reset(torch.from_numpy(done_h.astype(np.uint8)).to(b.device)).cpu().numpy()
      obs_h[done_h] = fresh[done_h]
    return obs_h, rew_h, done_h, infos

  def step(self, actions):
    self.step_async(actions)
    return self.step_wait()

  def close(self):
    pass

  def seed(self, seed=None):
    """Seeds are fixed at construction (``seed`` / ``seeds``): one RandomState per env, env.py:74."""
    return [None] * self.num_envs

  def reseed(self, seeds, episodes=None, indices=None):
    """BatchedEnv.reseed for the envs `indices` (all by default): seeds / episodes hold one entry per env named (episodes may be
    one int for all of them, default 1).  Takes effect at each env's next reset -- the one step_wait() does for it when its
    episode ends --, which starts episode `episodes` of that seed."""
    b = self._batch
    if indices is None:
      return b.reseed(seeds, episodes)
    idx = self._indices(indices)
    seeds = list(seeds)
    eps = [1 if episodes is None else episodes] * len(idx) if episodes is None or np.isscalar(episodes) else list(episodes)
    if len(seeds) != len(idx) or len(eps) != len(idx):
      raise ValueError('seeds and episodes need one entry per env named by indices')
    if any(not 0 <= i < self.num_envs for i in idx):
      raise ValueError(f'indices out of range 0 .. {self.num_envs - 1}')
    full_seeds, full_eps, mask = list(b.seeds), [1] * self.num_envs, np.zeros(self.num_envs, np.uint8)
    for i, s, e in zip(idx, seeds, eps):
      full_seeds[i], full_eps[i], mask[i] = s, e, 1
    return b.reseed(full_seeds, full_eps, mask)

  def set_levels(self, seeds, episodes=None, weights=None, key=0):
    """BatchedEnv.set_levels: the level table every env's coming resets draw from (None: clear).  Also reachable as
    ``env_method('set_levels', ...)``: the table belongs to the whole batch, `indices` is ignored."""
    return self._batch.set_levels(seeds, episodes, weights, key)

  def render(self, size=None, mode='rgb_array'):
    return self._batch.render(size).cpu().numpy()

  def get_images(self):
    return list(self.render())

  def _indices(self, indices):
    if indices is None:
      return list(range(self.num_envs))
    return [int(indices)] if np.isscalar(indices) else [int(i) for i in indices]

  def get_attr(self, attr_name, indices=None):
    return [getattr(self, attr_name) for _ in self._indices(indices)]

  def set_attr(self, attr_name, value, indices=None):
    raise AttributeError('the batched env has no per-env Python attributes to set')

  def action_masks(self):
    """bool [num_envs, n_actions]: BatchedEnv.legal_actions() of the states the next step() acts on (the SB3-contrib
    ``action_masks`` protocol of mask-aware trainers)."""
    return self._batch.legal_actions().cpu().numpy().astype(bool)

  def env_method(self, method_name, *args, indices=None, **kwargs):
    """``env_method('action_masks', indices=...)`` -> the list of rows SB3-contrib's ``get_action_masks`` stacks; there are
    no per-env Python objects to call anything else on, except ``env_method('set_levels', ...)``, which sets the batch's table."""
    if method_name == 'action_masks' and not args and not kwargs:
      masks = self.action_masks()
      return [masks[i] for i in self._indices(indices)]
    if method_name == 'set_levels':
      result = self.set_levels(*args, **kwargs)
      return [result for _ in self._indices(indices)]
    raise AttributeError('the batched env has no per-env Python objects to call')

  def env_is_wrapped(self, wrapper_class, indices=None):
    return [False for _ in self._indices(indices)]
