"""TEST INFRASTRUCTURE: the one builder of the CPU harness (no GPU needed).  Every target is one .cpp of this folder compiled
with g++ into tests/hostsim/_build/: the libraries that Python loads, and the stand-alone programs with
-fsanitize=address,undefined (sanitised code is never loaded into Python).  Also the helpers every wrapper module shares:
lib(), ptr(), fnv() and the writer of the blob the stand-alone programs read."""
import concurrent.futures
import ctypes as C
import pathlib
import struct
import subprocess

import numpy as np

from crafter_amd import abi

HERE = pathlib.Path(__file__).resolve().parent
ROOT = HERE.parent.parent
OUT_DIR = HERE / '_build'
MAX_JOBS = 16   # compilers at a time in build_all()

# CRAFTER_LIT_SPRITE_STEPS=96 (the library: 1024): one host thread lights the sprite-row table here; the scenarios run through
# both halves -- steps whose sprite rows come lit from the table and steps that light them per frame.
FLAGS = ['-std=c++17', '-g', '-ffp-contract=off', '-fno-fast-math', '-Wall', '-Wno-unused-variable', '-Wno-unknown-pragmas',
         '-D__device__=', '-D__host__=', '-D__forceinline__=inline', '-DCRAFTER_LIT_SPRITE_STEPS=96']
LIB_FLAGS = ['-O2', '-fPIC', '-shared']
# every check fatal: a finding ends the run with a non-zero status
SAN_FLAGS = ['-O1', '-fno-omit-frame-pointer', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']

# target -> its source; a new entry point is one row here
LIBS = {'hostsim': 'hostsim.cpp', 'symbolic': 'symbolic_host.cpp', 'final': 'final_host.cpp', 'levels': 'levels_host.cpp',
        'subset': 'subset_host.cpp', 'rollout_envs': 'rollout_envs_host.cpp', 'levelset': 'levelset_host.cpp',
        'worlds': 'worlds_host.cpp', 'legal': 'legal_host.cpp', 'generator_forms': 'generator_forms_host.cpp'}
PROGRAMS = {'final_main': 'final_main.cpp', 'worlds_main': 'worlds_main.cpp', 'legal_main': 'legal_main.cpp',
            'generator_forms_main': 'generator_forms_main.cpp'}

_libs = {}


def deps():
  """Every target depends on all of these: they include one another freely."""
  return sorted(HERE.glob('*.cpp')) + sorted(HERE.glob('*.hpp')) + sorted((ROOT / 'crafter_amd' / 'csrc').glob('*.hpp')) + [
      ROOT / 'include' / 'crafter_hip_types.h', ROOT / 'include' / 'crafter_hip.h']


def output(name, tag=''):
  if name in PROGRAMS:
    return OUT_DIR / f'{name}_san'
  stem = 'libhostsim' if name == 'hostsim' else f'libhostsim_{name}'
  return OUT_DIR / (f'{stem}_{tag}.so' if tag else f'{stem}.so')


def stale(out):
  return not out.exists() or out.stat().st_mtime < max(p.stat().st_mtime for p in deps())


def build(name='hostsim', defines=(), tag='', force=False):
  """Builds target `name` if it is older than a dependency -> its path.  defines / tag: a variant build of a library
  (e.g. CRAFTER_SPRITE_ROWS=1 under 'rows1', to force the renderer's overflow path)."""
  out = output(name, tag)
  if force or stale(out):
    src, mode = (PROGRAMS[name], SAN_FLAGS) if name in PROGRAMS else (LIBS[name], LIB_FLAGS)
    OUT_DIR.mkdir(exist_ok=True)
    subprocess.run(['g++'] + mode + FLAGS + [f'-D{d}' for d in defines] + ['-o', str(out), str(HERE / src)], check=True)
  return out


def build_all(force=False):
  """Every library, the stale ones compiled side by side -> their paths, in LIBS order.  (The sanitised programs are built
  by the tests that run them.)"""
  with concurrent.futures.ThreadPoolExecutor(MAX_JOBS) as pool:
    return list(pool.map(lambda name: build(name, force=force), LIBS))


def lib(name='hostsim', variant=None):
  """The loaded library of target `name`.  variant: None, or (tag, defines) for a differently configured build."""
  key = (name, variant)
  if key not in _libs:
    tag, defines = variant or ('', ())
    _libs[key] = C.CDLL(str(build(name, defines=defines, tag=tag)))
  return _libs[key]


def ptr(a):
  """numpy array -> void*; None -> NULL."""
  return None if a is None else a.ctypes.data_as(C.c_void_p)


def fnv(a):
  """FNV-1a over the array's bytes, as blob.hpp's."""
  h = 1469598103934665603
  for b in np.ascontiguousarray(a).view(np.uint8).ravel().tolist():
    h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
  return h


def write_blob(path, parts):
  """The stand-alone programs' input: each part (bytes) behind its length as a little-endian uint64 (blob.hpp reads it)."""
  with open(path, 'wb') as f:
    for p in parts:
      f.write(struct.pack('<Q', len(p)))
      f.write(p)


def env_parts(hs):
  """HostSimEnv `hs` as it stands, as blob parts: Config | the tables, in TablePtrs order | the state, in StatePtrs order
  (empty: null) -- what blob.hpp bind_env() takes."""
  t = hs.tab
  tabs = [hs._rules_buf, t.atlas, t.tex_tile, t.tex_icon, t.tex_digit, t.tex_alpha, t.item_pos, t.daylight, t.vignette, t.unit255, hs._static]
  names = [n for n, _ in abi.TablePtrs._fields_]
  assert names == ['rules', 'atlas', 'tex_tile', 'tex_icon', 'tex_digit', 'tex_alpha', 'item_pos', 'daylight', 'vignette', 'unit255', 'render_static']
  return [bytes(hs.cfg)] + [np.ascontiguousarray(x).tobytes() for x in tabs] + [
      hs.buf[name].tobytes() if name in hs.buf else b'' for name, _ in abi.StatePtrs._fields_]


if __name__ == '__main__':
  for path in build_all(force=True) + [build(name, force=True) for name in PROGRAMS]:
    print(path)
