"""TEST INFRASTRUCTURE: crafter_navigate's bodies on the CPU (navigate_host.cpp, built by tests/hostsim/build.py) over a
HostSimEnv's cfg / tb / st; and the stand-alone program of the same code (navigate_main.cpp, built with
-fsanitize=address,undefined), which reads a dumped HostSimEnv."""
import ctypes as C
import struct
import subprocess

import numpy as np

from crafter_amd import abi
from . import build as _build
from .build import ptr as _p

_build.LIBS.setdefault('navigate', 'navigate_host.cpp')
_build.PROGRAMS.setdefault('navigate_main', 'navigate_main.cpp')


def build_sanitized():
  return _build.build('navigate_main')


def lib():
  l = _build.lib('navigate')
  l.hostsim_navigate_error.restype = C.c_char_p
  return l


def map_is_state(hs):
  return bool(lib().hostsim_navigate_map_is_state(C.byref(hs.cfg)))


def in_registers(hs):
  return bool(lib().hostsim_navigate_in_registers(C.byref(hs.cfg)))


def call(hs, targets, k, passable, mask, dist, first, facing, force_map=-1):
  """hostsim_navigate with the arguments as given (numpy arrays or None) -> its return value."""
  return lib().hostsim_navigate(C.byref(hs.cfg), C.byref(hs.tb), C.byref(hs.st), _p(mask), _p(targets), C.c_int32(k), C.c_uint32(passable),
                                _p(dist), _p(first), _p(facing), C.c_int(force_map))


def error_text(reason):
  return lib().hostsim_navigate_error(C.c_int(reason)).decode()


def navigate(hs, targets, passable, mask=None, force_map=-1):
  """hostsim_navigate over HostSimEnv `hs`: targets (class sets as ints), passable (a material set) -> (dist int32 [N, K],
  first int32 [N, K], facing uint8 [N, K])."""
  n, k = hs.cfg.num_envs, len(targets)
  dist, first, facing = np.zeros((n, k), np.int32), np.zeros((n, k), np.int32), np.zeros((n, k), np.uint8)
  m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
  rc = call(hs, np.array(targets, np.uint32), k, passable, m, dist, first, facing, force_map)
  assert rc == 0, (rc, error_text(rc))
  return dist, first, facing


def dump(hs, path, targets, passable, mask=None, force_map=-1):
  """Writes what the bodies read of HostSimEnv `hs` (as it stands) and the query as the blob navigate_main.cpp reads."""
  parts = [bytes(hs.cfg), np.ascontiguousarray(hs._rules_buf).tobytes()] + [hs.buf[k].tobytes() for k in ('mat', 'objmap', 'objs', 'rec')]
  parts.append(b'' if mask is None else np.ascontiguousarray(mask, np.uint8).tobytes())
  sets = list(targets) + [0] * (abi.NAV_MAX_TARGETS - len(targets))
  parts.append(struct.pack('<17Iii', *sets, passable, len(targets), force_map))
  _build.write_blob(path, parts)


def run_sanitized(path):
  """-> the program's rows: per env None (row left untouched) or (dist, first, facing) lists of K ints."""
  proc = subprocess.run([str(build_sanitized()), str(path)], capture_output=True, text=True)
  assert proc.returncode == 0, proc.stderr[-3000:]
  rows = []
  for line in proc.stdout.splitlines():
    if line == '-':
      rows.append(None)
      continue
    v = [int(x) for x in line.split()]
    rows.append((v[0::3], v[1::3], v[2::3]))
  return rows
