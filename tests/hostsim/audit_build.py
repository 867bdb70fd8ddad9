"""TEST INFRASTRUCTURE: crafter_audit's body on the CPU (audit_host.cpp, built by tests/hostsim/build.py) over a HostSimEnv's
cfg / tb / st or over any dict of raw buffers laid out like them; and the stand-alone program of the same code (audit_main.cpp,
built with -fsanitize=address,undefined), which reads a dumped set of buffers."""
import ctypes as C
import struct
import subprocess

import numpy as np

from crafter_amd import abi
from . import build as _build
from .build import ptr as _p

_build.LIBS.setdefault('audit', 'audit_host.cpp')
_build.PROGRAMS.setdefault('audit_main', 'audit_main.cpp')

BUFFERS = ('mat', 'objmap', 'objs', 'rec', 'chunk_order', 'chunk_seen', 'census')   # what the body reads of a row


def build_sanitized():
  return _build.build('audit_main')


def lib():
  return _build.lib('audit')


def map_is_state(hs):
  """objmap is state for HostSimEnv `hs` (the maps stay in global memory)."""
  return not hs.lib.hostsim_slot_map_derived(C.byref(hs.cfg))


def copy_buffers(hs):
  """A private copy of the buffers the body reads, to corrupt."""
  return {k: hs.buf[k].copy() for k in BUFFERS}


def audit(hs, buf=None, mask=None, flags=None, detail=None, rc=0):
  """hostsim_audit over HostSimEnv `hs` (buf: other raw buffers of the same shapes in its place) -> (flags int32 [N],
  detail int32 [N, 4]).  rc: the return value to expect."""
  n = hs.cfg.num_envs
  flags = np.full(n, 0x7E7E7E7E, np.int32) if flags is None else flags
  detail = np.full((n, 4), 0x7E7E7E7E, np.int32) if detail is None else detail
  m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
  st = hs.st
  if buf is not None:
    st = abi.StatePtrs(**{name: (_p(buf[name]).value if name in buf else None) for name, _ in abi.StatePtrs._fields_})
  got = lib().hostsim_audit(C.byref(hs.cfg), C.byref(hs.tb), C.byref(st), int(map_is_state(hs)), _p(m), _p(flags), _p(detail))
  assert got == rc, got
  return flags, detail


def dump(hs, path, buf=None, mask=None):
  """Writes what the body reads (hs's buffers, or `buf`) as the blob audit_main.cpp reads."""
  buf = hs.buf if buf is None else buf
  state_map = map_is_state(hs)
  blob = [bytes(hs.cfg), np.ascontiguousarray(hs._rules_buf).tobytes(), struct.pack('<i', int(state_map))]
  blob += [b'' if (k == 'objmap' and not state_map) else np.ascontiguousarray(buf[k]).tobytes() for k in BUFFERS]
  blob.append(b'' if mask is None else np.ascontiguousarray(mask, np.uint8).tobytes())
  _build.write_blob(path, blob)


def run_sanitized(path):
  """-> the program's rows: per env None (row left untouched) or (flags, [the four detail words])."""
  proc = subprocess.run([str(build_sanitized()), str(path)], capture_output=True, text=True)
  assert proc.returncode == 0, proc.stderr[-3000:]
  rows = []
  for line in proc.stdout.splitlines():
    words = [int(x) for x in line.split()] if line != '-' else None
    rows.append(None if words is None else (words[0], words[1:]))
  return rows
