"""TEST INFRASTRUCTURE: builds tests/hostsim/_build/libhostsim_worlds.so (crafter_reset_worlds on the CPU, worlds_host.cpp) with
g++, with the flags of tests/hostsim/build.py, and runs it over a HostSimEnv's cfg / tb / st and a crafter_amd.WorldBank; and the
stand-alone program of the same code (worlds_main.cpp) with -fsanitize=address,undefined, which plays a dumped call."""
import ctypes as C
import pathlib
import struct
import subprocess

import numpy as np

from crafter_amd import abi

HERE = pathlib.Path(__file__).resolve().parent
OUT = HERE / '_build' / 'libhostsim_worlds.so'
OUT_SAN = HERE / '_build' / 'worlds_main_san'
SRCS = [HERE / 'worlds_host.cpp', HERE / 'worlds_main.cpp', HERE / 'wave_host.hpp'] + sorted(
    (HERE.parent.parent / 'crafter_amd' / 'csrc').glob('*.hpp')) + [HERE.parent.parent / 'include' / 'crafter_hip_types.h',
                                                                     HERE.parent.parent / 'include' / 'crafter_hip.h']
FLAGS = ['-std=c++17', '-g', '-ffp-contract=off', '-fno-fast-math', '-Wall', '-Wno-unused-variable', '-Wno-unknown-pragmas',
         '-D__device__=', '-D__host__=', '-D__forceinline__=inline', '-DCRAFTER_LIT_SPRITE_STEPS=96']

_lib = None


def _stale(out):
  return not out.exists() or out.stat().st_mtime < max(p.stat().st_mtime for p in SRCS)


def build(force=False):
  if force or _stale(OUT):
    OUT.parent.mkdir(exist_ok=True)
    subprocess.run(['g++', '-O2', '-fPIC', '-shared'] + FLAGS + ['-o', str(OUT), str(HERE / 'worlds_host.cpp')], check=True)
  return OUT


def build_sanitized(force=False):
  """The stand-alone program, every check fatal (a finding ends the run with a non-zero status)."""
  if force or _stale(OUT_SAN):
    OUT_SAN.parent.mkdir(exist_ok=True)
    subprocess.run(['g++', '-O1', '-fno-omit-frame-pointer', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'] + FLAGS +
                   ['-o', str(OUT_SAN), str(HERE / 'worlds_main.cpp')], check=True)
  return OUT_SAN


def lib():
  global _lib
  if _lib is None:
    _lib = C.CDLL(str(build()))
  return _lib


def _args(hs, bank, mask, world_ids):
  """The call's six arrays (None: NULL) and two sizes."""
  m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
  ids = None if world_ids is None else np.ascontiguousarray(world_ids, np.int32)
  assert m is None or m.size == hs.cfg.num_envs
  assert ids is None or ids.size == hs.cfg.num_envs
  objs = np.ascontiguousarray(bank.objs)
  return [m, ids, np.ascontiguousarray(bank.mat), objs, np.ascontiguousarray(bank.nobj),
          None if bank.inv is None else np.ascontiguousarray(bank.inv)], len(bank), int(objs.shape[1])


def reset_worlds(hs, bank, mask=None, world_ids=None):
  """hostsim_reset_worlds over HostSimEnv `hs` (its obs rows are written as by hs.reset) -> 0, or -1 for a host-side refusal."""
  arrays, n_worlds, cap = _args(hs, bank, mask, world_ids)
  p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
  return lib().hostsim_reset_worlds(C.byref(hs.cfg), C.byref(hs.tb), C.byref(hs.st), *[p(a) for a in arrays], n_worlds, cap, p(hs.obs))


def fnv(a):
  h = 1469598103934665603
  for b in np.ascontiguousarray(a).view(np.uint8).ravel().tolist():
    h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
  return h


def dump(hs, bank, path, mask=None, world_ids=None):
  """Writes HostSimEnv `hs` (as it stands) and the call's arguments as the blob worlds_main.cpp reads."""
  arrays, n_worlds, cap = _args(hs, bank, mask, world_ids)
  t = hs.tab
  tabs = [hs._rules_buf, t.atlas, t.tex_tile, t.tex_icon, t.tex_digit, t.tex_alpha, t.item_pos, t.daylight, t.vignette, t.unit255, hs._static]
  assert len(tabs) == len(abi.TablePtrs._fields_)
  parts = [struct.pack('<2i', n_worlds, cap), bytes(hs.cfg)]
  parts += [np.ascontiguousarray(x).tobytes() for x in tabs]
  for name, _ in abi.StatePtrs._fields_:
    parts.append(hs.buf[name].tobytes() if name in hs.buf else b'')
  parts += [b'' if a is None else a.tobytes() for a in arrays]
  with open(path, 'wb') as f:
    for p in parts:
      f.write(struct.pack('<Q', len(p)))
      f.write(p)


def lines(hs, mask=None):
  """What worlds_main.cpp prints for a call with `mask`, computed from HostSimEnv `hs`."""
  out = []
  for i in range(hs.cfg.num_envs):
    row = [fnv(hs.buf[k][i]) for k in ('mat', 'objs', 'mt', 'rec', 'chunk_order', 'census')] + [
        0 if mask is not None and not mask[i] else fnv(hs.obs[i])]
    out.append(f'{i} {int(hs.rec[i]["status"])} ' + ' '.join(f'{v:016x}' for v in row))
  return out


if __name__ == '__main__':
  print(build(force=True))
  print(build_sanitized(force=True))
