"""TEST INFRASTRUCTURE: builds tests/hostsim/_build/libhostsim_rollout_envs.so (crafter_step_n_envs on the CPU,
rollout_envs_host.cpp) with g++, with the flags of tests/hostsim/build.py, and runs it over a HostSimEnv's cfg / tb / st."""
import ctypes as C
import pathlib
import subprocess

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
OUT = HERE / '_build' / 'libhostsim_rollout_envs.so'
SRCS = [HERE / 'rollout_envs_host.cpp', HERE / 'wave_host.hpp'] + sorted((HERE.parent.parent / 'crafter_amd' / 'csrc').glob('*.hpp')) + [
    HERE.parent.parent / 'include' / 'crafter_hip_types.h']   # csrc/types.hpp includes it

_lib = None


def build(force=False):
  newest = max(p.stat().st_mtime for p in SRCS)
  if not force and OUT.exists() and OUT.stat().st_mtime >= newest:
    return OUT
  OUT.parent.mkdir(exist_ok=True)
  cmd = ['g++', '-std=c++17', '-O2', '-g', '-ffp-contract=off', '-fno-fast-math', '-fPIC', '-shared',
         '-Wall', '-Wno-unused-variable', '-Wno-unknown-pragmas', '-D__device__=', '-D__host__=',
         '-D__forceinline__=inline', '-DCRAFTER_LIT_SPRITE_STEPS=96', '-o', str(OUT), str(HERE / 'rollout_envs_host.cpp')]
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
  p = lambda x: x.ctypes.data_as(C.c_void_p)
  verdict = lib().hostsim_step_n_envs(C.byref(hs.cfg), C.byref(hs.tb), C.byref(hs.st), p(i), int(n), int(T), p(a), p(obs), p(reward), p(done),
                                      int(hs.pool), int(stretch), p(marks.words), marks.stamp)
  return verdict, obs, reward, done


if __name__ == '__main__':
  print(build(force=True))
