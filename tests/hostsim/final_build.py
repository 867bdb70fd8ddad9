"""TEST INFRASTRUCTURE: crafter_step_final on the CPU (final_host.cpp, built by tests/hostsim/build.py) over a HostSimEnv's
cfg / tb / st; and the stand-alone program of the same code (final_main.cpp, built with -fsanitize=address,undefined), which
plays a dumped HostSimEnv."""
import ctypes as C
import struct

import numpy as np

from . import build as _build
from .build import fnv, ptr as _p   # (fnv: the tests hash rows with it)


def build_sanitized():
  return _build.build('final_main')


def lib():
  return _build.lib('final')


class FinalBuffers:
  """The four outputs of crafter_step_final for a HostSimEnv, pre-filled with a pattern (rows of envs that did not finish stay)."""
  PATTERN, STATS_PATTERN = 0xA5, np.float32(-7)

  def __init__(self, hs):
    cfg = hs.cfg
    n = cfg.num_envs
    self.obs = np.full((n, cfg.size_h, cfg.size_w, 3), self.PATTERN, np.uint8)
    self.terminated = np.full(n, self.PATTERN, np.uint8)
    self.local = np.full((n, 2, cfg.local_gw, cfg.local_gh), self.PATTERN, np.uint8)
    self.stats = np.full((n, hs.tab.rules.n_items + 4), self.STATS_PATTERN, np.float32)


def step_final(hs, actions, fin, split=False):
  """hostsim_step_final over HostSimEnv `hs` (its obs / reward / done are written as by hs.step) -> envs that came through the queue."""
  a = np.ascontiguousarray(actions, np.int32)
  rc = lib().hostsim_step_final(C.byref(hs.cfg), C.byref(hs.tb), C.byref(hs.st), _p(a), _p(hs.obs), _p(hs.reward), _p(hs.done), int(hs.pool), int(split),
                                _p(fin.obs if hs.cfg.render_obs else None), _p(fin.terminated), _p(fin.local), _p(fin.stats))
  return rc


def dump(hs, actions, path, split=False):
  """Writes HostSimEnv `hs` (as it stands) and the tape actions [T, N] as the blob final_main.cpp reads."""
  acts = np.ascontiguousarray(actions, np.int32)
  _build.write_blob(path, [struct.pack('<3i', acts.shape[0], int(hs.pool), int(split))] + _build.env_parts(hs) + [acts.tobytes()])
