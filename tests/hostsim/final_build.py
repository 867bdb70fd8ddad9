"""TEST INFRASTRUCTURE: builds tests/hostsim/_build/libhostsim_final.so (crafter_step_final on the CPU, final_host.cpp) with
g++, with the flags of tests/hostsim/build.py, and runs it over a HostSimEnv's cfg / tb / st; and the stand-alone program of the
same code (final_main.cpp) with -fsanitize=address,undefined, which plays a dumped HostSimEnv."""
import ctypes as C
import pathlib
import struct
import subprocess

import numpy as np

from crafter_amd import abi

HERE = pathlib.Path(__file__).resolve().parent
OUT = HERE / '_build' / 'libhostsim_final.so'
OUT_SAN = HERE / '_build' / 'final_main_san'
SRCS = [HERE / 'final_host.cpp', HERE / 'final_main.cpp', HERE / 'wave_host.hpp'] + sorted(
    (HERE.parent.parent / 'crafter_amd' / 'csrc').glob('*.hpp')) + [HERE.parent.parent / 'include' / 'crafter_hip_types.h']
FLAGS = ['-std=c++17', '-g', '-ffp-contract=off', '-fno-fast-math', '-Wall', '-Wno-unused-variable', '-Wno-unknown-pragmas',
         '-D__device__=', '-D__host__=', '-D__forceinline__=inline', '-DCRAFTER_LIT_SPRITE_STEPS=96']

_lib = None


def _stale(out):
  return not out.exists() or out.stat().st_mtime < max(p.stat().st_mtime for p in SRCS)


def build(force=False):
  if force or _stale(OUT):
    OUT.parent.mkdir(exist_ok=True)
    subprocess.run(['g++', '-O2', '-fPIC', '-shared'] + FLAGS + ['-o', str(OUT), str(HERE / 'final_host.cpp')], check=True)
  return OUT


def build_sanitized(force=False):
  """The stand-alone program, every check fatal (a finding ends the run with a non-zero status)."""
  if force or _stale(OUT_SAN):
    OUT_SAN.parent.mkdir(exist_ok=True)
    subprocess.run(['g++', '-O1', '-fno-omit-frame-pointer', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'] + FLAGS +
                   ['-o', str(OUT_SAN), str(HERE / 'final_main.cpp')], check=True)
  return OUT_SAN


def lib():
  global _lib
  if _lib is None:
    _lib = C.CDLL(str(build()))
  return _lib


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
  p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
  rc = lib().hostsim_step_final(C.byref(hs.cfg), C.byref(hs.tb), C.byref(hs.st), p(a), p(hs.obs), p(hs.reward), p(hs.done), int(hs.pool), int(split),
                                p(fin.obs if hs.cfg.render_obs else None), p(fin.terminated), p(fin.local), p(fin.stats))
  return rc


def fnv(a):
  h = 1469598103934665603
  for b in np.ascontiguousarray(a).view(np.uint8).ravel().tolist():
    h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
  return h


def dump(hs, actions, path, split=False):
  """Writes HostSimEnv `hs` (as it stands) and the tape actions [T, N] as the blob final_main.cpp reads."""
  acts = np.ascontiguousarray(actions, np.int32)
  t = hs.tab
  tables = [hs._rules_buf, t.atlas, t.tex_tile, t.tex_icon, t.tex_digit, t.tex_alpha, t.item_pos, t.daylight, t.vignette, t.unit255, hs._static]
  names = [n for n, _ in abi.TablePtrs._fields_]
  assert names == ['rules', 'atlas', 'tex_tile', 'tex_icon', 'tex_digit', 'tex_alpha', 'item_pos', 'daylight', 'vignette', 'unit255', 'render_static']
  parts = [struct.pack('<3i', acts.shape[0], int(hs.pool), int(split)), bytes(hs.cfg)]
  parts += [np.ascontiguousarray(x).tobytes() for x in tables]
  for name, _ in abi.StatePtrs._fields_:
    parts.append(hs.buf[name].tobytes() if name in hs.buf else b'')
  parts.append(acts.tobytes())
  with open(path, 'wb') as f:
    for p in parts:
      f.write(struct.pack('<Q', len(p)))
      f.write(p)


if __name__ == '__main__':
  print(build(force=True))
  print(build_sanitized(force=True))
