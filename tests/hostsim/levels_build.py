"""TEST INFRASTRUCTURE: builds tests/hostsim/_build/libhostsim_levels.so (crafter_reseed's body on the CPU, levels_host.cpp) with
g++, with the flags of tests/hostsim/build.py, and runs it over a HostSimEnv's cfg / st or over hand-made ones."""
import ctypes as C
import pathlib
import subprocess

import numpy as np

from crafter_amd import state

HERE = pathlib.Path(__file__).resolve().parent
OUT = HERE / '_build' / 'libhostsim_levels.so'
SRCS = [HERE / 'levels_host.cpp', HERE / 'wave_host.hpp'] + sorted((HERE.parent.parent / 'crafter_amd' / 'csrc').glob('*.hpp')) + [
    HERE.parent.parent / 'include' / 'crafter_hip_types.h']   # csrc/types.hpp includes it

_lib = None


def build(force=False):
  newest = max(p.stat().st_mtime for p in SRCS)
  if not force and OUT.exists() and OUT.stat().st_mtime >= newest:
    return OUT
  OUT.parent.mkdir(exist_ok=True)
  cmd = ['g++', '-std=c++17', '-O2', '-g', '-ffp-contract=off', '-fno-fast-math', '-fPIC', '-shared',
         '-Wall', '-Wno-unused-variable', '-Wno-unknown-pragmas', '-D__device__=', '-D__host__=',
         '-D__forceinline__=inline', '-o', str(OUT), str(HERE / 'levels_host.cpp')]
  subprocess.run(cmd, check=True)
  return OUT


def lib():
  global _lib
  if _lib is None:
    _lib = C.CDLL(str(build()))
  return _lib


def reseed_raw(cfg, st, mask, lanes, episodes):
  """hostsim_reseed over any (Config, StatePtrs); mask / episodes may be None.  The arrays are passed as they are."""
  p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
  rc = lib().hostsim_reseed(C.byref(cfg), C.byref(st), p(mask), p(lanes), p(episodes))
  assert rc == 0


def reseed(hs, seeds, episodes=None, mask=None):
  """BatchedEnv.reseed on HostSimEnv `hs`: host seeds (one per env) hashed as the product hashes them."""
  lanes = state.seed_lanes(seeds)
  assert lanes.size == hs.cfg.num_envs
  eps = None if episodes is None else np.ascontiguousarray(np.broadcast_to(np.asarray(episodes, np.int32), (hs.cfg.num_envs,)))
  m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
  reseed_raw(hs.cfg, hs.st, m, lanes, eps)


if __name__ == '__main__':
  print(build(force=True))
