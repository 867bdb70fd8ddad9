"""TEST INFRASTRUCTURE: builds tests/hostsim/_build/libhostsim_legal.so (crafter_legal_actions' body on the CPU) with g++, with
the flags of tests/hostsim/build.py, and runs it over a HostSimEnv's cfg / tb / st; and the stand-alone program of the same
code (legal_main.cpp) with -fsanitize=address,undefined, which reads a dumped HostSimEnv."""
import ctypes as C
import pathlib
import struct
import subprocess

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
OUT = HERE / '_build' / 'libhostsim_legal.so'
OUT_SAN = HERE / '_build' / 'legal_main_san'
SRCS = [HERE / 'legal_host.cpp', HERE / 'legal_main.cpp', HERE / 'wave_host.hpp'] + sorted(
    (HERE.parent.parent / 'crafter_amd' / 'csrc').glob('*.hpp')) + [HERE.parent.parent / 'include' / 'crafter_hip_types.h']
FLAGS = ['-std=c++17', '-g', '-ffp-contract=off', '-fno-fast-math', '-Wall', '-Wno-unused-variable', '-Wno-unknown-pragmas',
         '-D__device__=', '-D__host__=', '-D__forceinline__=inline', '-DCRAFTER_LIT_SPRITE_STEPS=96']

_lib = None


def _stale(out):
  return not out.exists() or out.stat().st_mtime < max(p.stat().st_mtime for p in SRCS)


def build(force=False):
  if force or _stale(OUT):
    OUT.parent.mkdir(exist_ok=True)
    subprocess.run(['g++', '-O2', '-fPIC', '-shared'] + FLAGS + ['-o', str(OUT), str(HERE / 'legal_host.cpp')], check=True)
  return OUT


def build_sanitized(force=False):
  """The stand-alone program, every check fatal (a finding ends the run with a non-zero status)."""
  if force or _stale(OUT_SAN):
    OUT_SAN.parent.mkdir(exist_ok=True)
    subprocess.run(['g++', '-O1', '-fno-omit-frame-pointer', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'] + FLAGS +
                   ['-o', str(OUT_SAN), str(HERE / 'legal_main.cpp')], check=True)
  return OUT_SAN


def lib():
  global _lib
  if _lib is None:
    _lib = C.CDLL(str(build()))
  return _lib


def legal(hs, mask=None, out=None):
  """hostsim_legal over HostSimEnv `hs` -> legal u8 [N, n_actions]."""
  cfg = hs.cfg
  if out is None:
    out = np.zeros((cfg.num_envs, hs.tab.rules.n_actions), np.uint8)
  m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
  p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
  rc = lib().hostsim_legal(C.byref(cfg), C.byref(hs.tb), C.byref(hs.st), p(m), p(out))
  assert rc == 0
  return out


def map_is_state(hs):
  return bool(lib().hostsim_legal_map_is_state(C.byref(hs.cfg)))


def dump(hs, path, mask=None):
  """Writes what the body reads of HostSimEnv `hs` (as it stands) as the blob legal_main.cpp reads."""
  parts = [bytes(hs.cfg), np.ascontiguousarray(hs._rules_buf).tobytes()] + [hs.buf[k].tobytes() for k in ('mat', 'objmap', 'objs', 'rec')]
  parts.append(b'' if mask is None else np.ascontiguousarray(mask, np.uint8).tobytes())
  with open(path, 'wb') as f:
    for p in parts:
      f.write(struct.pack('<Q', len(p)))
      f.write(p)


def run_sanitized(path):
  """-> the program's rows: uint8 [N, n_actions], 0xFF where a row was left untouched."""
  proc = subprocess.run([str(build_sanitized()), str(path)], capture_output=True, text=True)
  assert proc.returncode == 0, proc.stderr[-3000:]
  return np.array([[0xFF if c == '-' else int(c) for c in line] for line in proc.stdout.split()], np.uint8)


if __name__ == '__main__':
  print(build(force=True))
  print(build_sanitized(force=True))
