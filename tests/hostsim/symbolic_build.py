"""TEST INFRASTRUCTURE: builds tests/hostsim/_build/libhostsim_symbolic.so (crafter_symbolic's body on the CPU) with g++,
with the flags of tests/hostsim/build.py, and runs it over a HostSimEnv's cfg / tb / st."""
import ctypes as C
import pathlib
import subprocess

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
OUT = HERE / '_build' / 'libhostsim_symbolic.so'
SRCS = [HERE / 'symbolic_host.cpp', HERE / 'wave_host.hpp'] + sorted((HERE.parent.parent / 'crafter_amd' / 'csrc').glob('*.hpp')) + [
    HERE.parent.parent / 'include' / 'crafter_hip_types.h']   # csrc/types.hpp includes it

_lib = None


def build(force=False):
  newest = max(p.stat().st_mtime for p in SRCS)
  if not force and OUT.exists() and OUT.stat().st_mtime >= newest:
    return OUT
  OUT.parent.mkdir(exist_ok=True)
  cmd = ['g++', '-std=c++17', '-O2', '-g', '-ffp-contract=off', '-fno-fast-math', '-fPIC', '-shared',
         '-Wall', '-Wno-unused-variable', '-Wno-unknown-pragmas', '-D__device__=', '-D__host__=',
         '-D__forceinline__=inline', '-DCRAFTER_LIT_SPRITE_STEPS=96', '-o', str(OUT), str(HERE / 'symbolic_host.cpp')]
  subprocess.run(cmd, check=True)
  return OUT


def lib():
  global _lib
  if _lib is None:
    _lib = C.CDLL(str(build()))
  return _lib


def symbolic(hs, mask=None, out=None):
  """hostsim_symbolic over HostSimEnv `hs` -> (local u8 [N, 2, gw, gh], stats f32 [N, n_items + 4])."""
  cfg = hs.cfg
  n, ni = cfg.num_envs, hs.tab.rules.n_items
  if out is None:
    out = (np.zeros((n, 2, cfg.local_gw, cfg.local_gh), np.uint8), np.zeros((n, ni + 4), np.float32))
  local, stats = out
  m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
  p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
  rc = lib().hostsim_symbolic(C.byref(cfg), C.byref(hs.tb), C.byref(hs.st), p(m), p(local), p(stats))
  assert rc == 0
  return local, stats


def map_is_state(hs):
  return bool(lib().hostsim_symbolic_map_is_state(C.byref(hs.cfg)))


if __name__ == '__main__':
  print(build(force=True))
