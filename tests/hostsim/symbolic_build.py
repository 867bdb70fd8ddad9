"""TEST INFRASTRUCTURE: crafter_symbolic's body on the CPU (symbolic_host.cpp, built by tests/hostsim/build.py) over a HostSimEnv's
cfg / tb / st."""
import ctypes as C

import numpy as np

from . import build as _build
from .build import ptr as _p


def lib():
  return _build.lib('symbolic')


def symbolic(hs, mask=None, out=None):
  """hostsim_symbolic over HostSimEnv `hs` -> (local u8 [N, 2, gw, gh], stats f32 [N, n_items + 4])."""
  cfg = hs.cfg
  n, ni = cfg.num_envs, hs.tab.rules.n_items
  if out is None:
    out = (np.zeros((n, 2, cfg.local_gw, cfg.local_gh), np.uint8), np.zeros((n, ni + 4), np.float32))
  local, stats = out
  m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
  rc = lib().hostsim_symbolic(C.byref(cfg), C.byref(hs.tb), C.byref(hs.st), _p(m), _p(local), _p(stats))
  assert rc == 0
  return local, stats


def map_is_state(hs):
  return bool(lib().hostsim_symbolic_map_is_state(C.byref(hs.cfg)))
