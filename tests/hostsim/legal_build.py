"""TEST INFRASTRUCTURE: crafter_legal_actions' body on the CPU (legal_host.cpp, built by tests/hostsim/build.py) over a
HostSimEnv's cfg / tb / st; and the stand-alone program of the same code (legal_main.cpp, built with
-fsanitize=address,undefined), which reads a dumped HostSimEnv."""
import ctypes as C
import subprocess

import numpy as np

from . import build as _build
from .build import ptr as _p


def build_sanitized():
  return _build.build('legal_main')


def lib():
  return _build.lib('legal')


def legal(hs, mask=None, out=None):
  """hostsim_legal over HostSimEnv `hs` -> legal u8 [N, n_actions]."""
  cfg = hs.cfg
  if out is None:
    out = np.zeros((cfg.num_envs, hs.tab.rules.n_actions), np.uint8)
  m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
  rc = lib().hostsim_legal(C.byref(cfg), C.byref(hs.tb), C.byref(hs.st), _p(m), _p(out))
  assert rc == 0
  return out


def map_is_state(hs):
  return bool(lib().hostsim_legal_map_is_state(C.byref(hs.cfg)))


def dump(hs, path, mask=None):
  """Writes what the body reads of HostSimEnv `hs` (as it stands) as the blob legal_main.cpp reads."""
  parts = [bytes(hs.cfg), np.ascontiguousarray(hs._rules_buf).tobytes()] + [hs.buf[k].tobytes() for k in ('mat', 'objmap', 'objs', 'rec')]
  parts.append(b'' if mask is None else np.ascontiguousarray(mask, np.uint8).tobytes())
  _build.write_blob(path, parts)


def run_sanitized(path):
  """-> the program's rows: uint8 [N, n_actions], 0xFF where a row was left untouched."""
  proc = subprocess.run([str(build_sanitized()), str(path)], capture_output=True, text=True)
  assert proc.returncode == 0, proc.stderr[-3000:]
  return np.array([[0xFF if c == '-' else int(c) for c in line] for line in proc.stdout.split()], np.uint8)
