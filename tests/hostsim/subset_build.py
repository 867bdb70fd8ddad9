"""TEST INFRASTRUCTURE: crafter_step_envs on the CPU (subset_host.cpp, built by tests/hostsim/build.py) over a HostSimEnv's
cfg / tb / st."""
import ctypes as C

import numpy as np

from . import build as _build
from .build import ptr as _p


def lib():
  return _build.lib('subset')


class Marks:
  """The index check's scratch of one handle: a mark per env, the verdict word, the call counter."""

  def __init__(self, num_envs):
    self.words = np.zeros(num_envs + 1, np.int32)
    self.stamp = 0


def step_envs(hs, marks, idx, actions):
  """hostsim_step_envs over HostSimEnv `hs` (its obs / reward / done rows are written as by hs.step) -> the verdict."""
  i = np.ascontiguousarray(idx, np.int32)
  a = np.ascontiguousarray(actions, np.int32)
  assert i.ndim == 1 and a.shape == i.shape
  marks.stamp += 1
  return lib().hostsim_step_envs(C.byref(hs.cfg), C.byref(hs.tb), C.byref(hs.st), _p(i), int(i.size), _p(a), _p(hs.obs), _p(hs.reward), _p(hs.done),
                                 int(hs.pool), _p(marks.words), marks.stamp)


def choose(cfg, default_rules, n, frames, wide):
  """-> (kernel: 0 fused / 1 wide, instance) of launch_plan.hpp choose_step_envs."""
  inst = C.c_int32()
  k = lib().hostsim_choose_step_envs(C.byref(cfg), int(default_rules), int(n), int(frames), int(wide), C.byref(inst))
  return k, inst.value
