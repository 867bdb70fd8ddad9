"""TEST INFRASTRUCTURE: builds tests/hostsim/_build/libhostsim_subset.so (crafter_step_envs on the CPU, subset_host.cpp) with
g++, with the flags of tests/hostsim/build.py, and runs it over a HostSimEnv's cfg / tb / st."""
import ctypes as C
import pathlib
import subprocess

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
OUT = HERE / '_build' / 'libhostsim_subset.so'
SRCS = [HERE / 'subset_host.cpp', HERE / 'wave_host.hpp'] + sorted((HERE.parent.parent / 'crafter_amd' / 'csrc').glob('*.hpp')) + [
    HERE.parent.parent / 'include' / 'crafter_hip_types.h']   # csrc/types.hpp includes it

_lib = None


def build(force=False):
  newest = max(p.stat().st_mtime for p in SRCS)
  if not force and OUT.exists() and OUT.stat().st_mtime >= newest:
    return OUT
  OUT.parent.mkdir(exist_ok=True)
  cmd = ['g++', '-std=c++17', '-O2', '-g', '-ffp-contract=off', '-fno-fast-math', '-fPIC', '-shared',
         '-Wall', '-Wno-unused-variable', '-Wno-unknown-pragmas', '-D__device__=', '-D__host__=',
         '-D__forceinline__=inline', '-DCRAFTER_LIT_SPRITE_STEPS=96', '-o', str(OUT), str(HERE / 'subset_host.cpp')]
  subprocess.run(cmd, check=True)
  return OUT


def lib():
  global _lib
  if _lib is None:
    _lib = C.CDLL(str(build()))
  return _lib


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
  p = lambda x: x.ctypes.data_as(C.c_void_p)
  return lib().hostsim_step_envs(C.byref(hs.cfg), C.byref(hs.tb), C.byref(hs.st), p(i), int(i.size), p(a), p(hs.obs), p(hs.reward), p(hs.done),
                                 int(hs.pool), p(marks.words), marks.stamp)


def choose(cfg, default_rules, n, frames, wide):
  """-> (kernel: 0 fused / 1 wide, instance) of launch_plan.hpp choose_step_envs."""
  inst = C.c_int32()
  k = lib().hostsim_choose_step_envs(C.byref(cfg), int(default_rules), int(n), int(frames), int(wide), C.byref(inst))
  return k, inst.value


if __name__ == '__main__':
  print(build(force=True))
