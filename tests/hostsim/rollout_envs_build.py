"""TEST INFRASTRUCTURE: crafter_step_n_envs on the CPU (rollout_envs_host.cpp, built by tests/hostsim/build.py) over a
HostSimEnv's cfg / tb / st."""
import ctypes as C

import numpy as np

from . import build as _build
from .build import ptr as _p


def lib():
  return _build.lib('rollout_envs')


class Marks:
  """The index check's scratch of one handle: a mark per env, the verdict word, the call counter."""

  def __init__(self, num_envs):
    self.words = np.zeros(num_envs + 1, np.int32)
    self.stamp = 0


def rollout_envs(hs, marks, idx, actions, out=None, stretch=16):
  """hostsim_step_n_envs over HostSimEnv `hs`: actions [T, n] -> (verdict, obs [T, n, h, w, 3], reward [T, n], done [T, n]).
  out: (obs, reward, done) arrays of those shapes to write into."""
  i = np.ascontiguousarray(idx, np.int32)
  a = np.ascontiguousarray(actions, np.int32)
  assert i.ndim == 1 and a.ndim == 2 and a.shape[1] == i.size
  T, n = a.shape
  if out is None:
    out = (np.zeros((T, n) + hs.obs.shape[1:], np.uint8), np.zeros((T, n), np.float32), np.zeros((T, n), np.uint8))
  obs, reward, done = out
  assert obs.shape == (T, n) + hs.obs.shape[1:] and reward.shape == (T, n) and done.shape == (T, n)
  marks.stamp += 1
  verdict = lib().hostsim_step_n_envs(C.byref(hs.cfg), C.byref(hs.tb), C.byref(hs.st), _p(i), int(n), int(T), _p(a), _p(obs), _p(reward), _p(done),
                                      int(hs.pool), int(stretch), _p(marks.words), marks.stamp)
  return verdict, obs, reward, done
