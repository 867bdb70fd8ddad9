"""TEST INFRASTRUCTURE: crafter_reseed's body on the CPU (levels_host.cpp, built by tests/hostsim/build.py) over a HostSimEnv's
cfg / st or over hand-made ones."""
import ctypes as C

import numpy as np

from crafter_amd import state
from . import build as _build
from .build import ptr as _p


def lib():
  return _build.lib('levels')


def reseed_raw(cfg, st, mask, lanes, episodes):
  """hostsim_reseed over any (Config, StatePtrs); mask / episodes may be None.  The arrays are passed as they are."""
  rc = lib().hostsim_reseed(C.byref(cfg), C.byref(st), _p(mask), _p(lanes), _p(episodes))
  assert rc == 0


def reseed(hs, seeds, episodes=None, mask=None):
  """BatchedEnv.reseed on HostSimEnv `hs`: host seeds (one per env) hashed as the product hashes them."""
  lanes = state.seed_lanes(seeds)
  assert lanes.size == hs.cfg.num_envs
  eps = None if episodes is None else np.ascontiguousarray(np.broadcast_to(np.asarray(episodes, np.int32), (hs.cfg.num_envs,)))
  m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
  reseed_raw(hs.cfg, hs.st, m, lanes, eps)
