"""TEST INFRASTRUCTURE: the level-set bodies of csrc/env_levels.hpp and the reset / step walks with a level table on the CPU
(levelset_host.cpp, built by tests/hostsim/build.py)."""
import ctypes as C

import numpy as np

from crafter_amd import state
from .driver import HostSimEnv
from . import build as _build
from .build import ptr as _p


def lib():
  l = _build.lib('levelset')
  l.hostsim_level_table_bytes.restype = C.c_longlong
  l.hostsim_level_seed.restype = C.c_uint32
  l.hostsim_level_seed.argtypes = [C.c_void_p, C.c_uint64, C.c_int]
  l.hostsim_set_levels.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_uint64]
  return l


class Table:
  """A LevelTable in host memory, full of noise until set() (the kernel reads nothing it has not written)."""

  def __init__(self):
    self.buf = np.random.RandomState(11).randint(0, 256, size=int(lib().hostsim_level_table_bytes())).astype(np.uint8)
    self.K, self.cum, self.key = 0, None, 0

  @property
  def ptr(self):
    return _p(self.buf)

  def set(self, cfg, st, lanes, episodes, cum=None, key=0):
    """hostsim_set_levels over (cfg, st): arrays as the C call takes them (lanes uint64, episodes int32, cum uint32 or None)."""
    K = 0 if lanes is None else len(lanes)
    rc = lib().hostsim_set_levels(C.cast(C.byref(cfg), C.c_void_p), C.cast(C.byref(st), C.c_void_p), self.ptr, _p(lanes), _p(episodes), _p(cum),
                                  K, int(key) & 0xFFFFFFFFFFFFFFFF)
    assert rc == 0
    self.K, self.cum, self.key = K, cum, key

  def pick(self, lanes, k):
    lanes = np.ascontiguousarray(lanes, np.uint64)
    k = np.ascontiguousarray(k, np.int32)
    out = np.full(lanes.size, -7, np.int32)
    lib().hostsim_level_pick(self.ptr, _p(lanes), _p(k), _p(out), int(lanes.size))
    return out

  def ids(self, cfg, st, mask=None, table=True, fill=-5):
    out = np.full(cfg.num_envs, fill, np.int32)
    rc = lib().hostsim_level_ids(C.byref(cfg), C.byref(st), self.ptr if table else None, _p(mask), _p(out))
    assert rc == 0
    return out


class LevelSetEnv(HostSimEnv):
  """HostSimEnv whose reset() / step() hand a level table to the bodies that seed a world."""

  def __init__(self, *a, **kw):
    super().__init__(*a, **kw)
    self.table = Table()
    self.table.set(self.cfg, self.st, None, None)   # no table: n = 0

  def set_levels(self, seeds, episodes=None, cum=None, key=0):
    if seeds is None:
      return self.table.set(self.cfg, self.st, None, None)
    lanes = state.seed_lanes(seeds)
    eps = np.ones(len(seeds), np.int32) if episodes is None else np.ascontiguousarray(episodes, np.int32)
    self.table.set(self.cfg, self.st, lanes, eps, cum, key)

  def level_ids(self):
    return self.table.ids(self.cfg, self.st)

  def reset(self, mask=None):
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    rc = lib().hostsim_levelset_reset(C.byref(self.cfg), C.byref(self.tb), C.byref(self.st), self.table.ptr, _p(m), self.pool, _p(self.obs))
    assert rc == 0
    return self.obs

  def step(self, actions):
    a = np.ascontiguousarray(actions, np.int32)
    rc = lib().hostsim_levelset_step(C.byref(self.cfg), C.byref(self.tb), C.byref(self.st), self.table.ptr, _p(a), _p(self.obs),
                                     _p(self.reward), _p(self.done), self.pool)
    assert rc == 0
    return self.obs, self.reward, self.done
