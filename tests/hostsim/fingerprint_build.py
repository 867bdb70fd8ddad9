"""TEST INFRASTRUCTURE: crafter_fingerprint's body on the CPU (fingerprint_host.cpp, built by tests/hostsim/build.py) over a
HostSimEnv's cfg / tb / st; and the stand-alone program of the same code (fingerprint_main.cpp, built with
-fsanitize=address,undefined), which reads a dumped HostSimEnv."""
import ctypes as C
import struct
import subprocess

import numpy as np

from crafter_amd import abi
from . import build as _build
from .build import ptr as _p

_build.LIBS.setdefault('fingerprint', 'fingerprint_host.cpp')
_build.PROGRAMS.setdefault('fingerprint_main', 'fingerprint_main.cpp')


def build_sanitized():
  return _build.build('fingerprint_main')


def lib():
  return _build.lib('fingerprint')


def fingerprint(hs, parts=abi.FP_ALL, mask=None, key=None, part_hash=None, rc=0):
  """hostsim_fingerprint over HostSimEnv `hs` -> (key uint64 [N], part_hash uint64 [N, 7]).  rc: the return value to expect."""
  n = hs.cfg.num_envs
  key = np.zeros(n, np.uint64) if key is None else key
  part_hash = np.zeros((n, abi.FP_PARTS), np.uint64) if part_hash is None else part_hash
  m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
  got = lib().hostsim_fingerprint(C.byref(hs.cfg), C.byref(hs.tb), C.byref(hs.st), _p(m), C.c_uint32(parts), _p(key), _p(part_hash))
  assert got == rc, got
  return key, part_hash


def dump(hs, path, parts=abi.FP_ALL, mask=None):
  """Writes what the body reads of HostSimEnv `hs` (as it stands) as the blob fingerprint_main.cpp reads."""
  blob = [bytes(hs.cfg), np.ascontiguousarray(hs._rules_buf).tobytes()] + [hs.buf[k].tobytes() for k in ('mat', 'objs', 'mt', 'rec', 'chunk_order')]
  blob.append(b'' if mask is None else np.ascontiguousarray(mask, np.uint8).tobytes())
  blob.append(struct.pack('<I', parts))
  _build.write_blob(path, blob)


def run_sanitized(path):
  """-> the program's rows: a list with, per env, None (row left untouched) or (key, [the seven part hashes])."""
  proc = subprocess.run([str(build_sanitized()), str(path)], capture_output=True, text=True)
  assert proc.returncode == 0, proc.stderr[-3000:]
  rows = []
  for line in proc.stdout.splitlines():
    words = [int(x, 16) for x in line.split()] if line != '-' else None
    rows.append(None if words is None else (words[0], words[1:]))
  return rows
