"""TEST INFRASTRUCTURE: crafter_edit_envs on the CPU (edits_host.cpp, built by tests/hostsim/build.py) over a HostSimEnv's
cfg / tb / st and a tape of crafter_amd.edits; and the stand-alone program of the same code (edits_main.cpp, built with
-fsanitize=address,undefined), which plays a dumped call."""
import ctypes as C
import struct

import numpy as np

from crafter_amd import edits
from . import build as _build
from .build import fnv, ptr as _p

_build.LIBS.setdefault('edits', 'edits_host.cpp')
_build.PROGRAMS.setdefault('edits_main', 'edits_main.cpp')

BUFFERS = ('mat', 'objmap', 'objs', 'mt', 'rec', 'chunk_order', 'chunk_seen', 'census')


def build_sanitized():
  return _build.build('edits_main')


def lib():
  return _build.lib('edits')


def lds_bytes(hs):
  return int(lib().hostsim_edit_lds_bytes(C.byref(hs.cfg)))


def _marks(hs):
  """The index check's marks and verdict word and the call counter, kept with the HostSimEnv as the library keeps them with its handle."""
  if not hasattr(hs, '_edit_marks'):
    hs._edit_marks, hs._edit_stamp = np.zeros(hs.cfg.num_envs + 1, np.int32), 0
  return hs._edit_marks


def tape_of(hs, idx, ops, validate=True):
  """ops as BatchedEnv.edit takes them (a tape, n tapes, or an int array [n, L, 8]) -> contiguous np.int32 [n, L, 8]."""
  if isinstance(ops, np.ndarray):
    return np.ascontiguousarray(ops, np.int32).reshape(len(idx), -1, edits.WORDS)
  return edits.encode(hs, ops, len(idx), validate=validate)


def edit(hs, idx, ops, validate=True, next_step=None):
  """hostsim_edit_envs over HostSimEnv `hs` -> the verdict (0: edited, 1: the index list was refused), or -1 for a host-side refusal."""
  idx = np.ascontiguousarray(idx, np.int32)
  tape = tape_of(hs, idx, ops, validate)
  mark = _marks(hs)
  hs._edit_stamp += 1
  return lib().hostsim_edit_envs(C.byref(hs.cfg), C.byref(hs.tb), C.byref(hs.st), _p(idx), len(idx), _p(tape), int(tape.shape[1]), _p(mark),
                                 hs._edit_stamp, _p(next_step))


def dump(hs, path, idx, ops, validate=True):
  """Writes HostSimEnv `hs` (as it stands) and the call's arguments as the blob edits_main.cpp reads."""
  idx = np.ascontiguousarray(idx, np.int32)
  tape = tape_of(hs, idx, ops, validate)
  _build.write_blob(path, [struct.pack('<3i', len(idx), int(tape.shape[1]), 1)] + _build.env_parts(hs) + [
      idx.tobytes(), tape.tobytes(), np.zeros(hs.cfg.num_envs + 1, np.int32).tobytes()])


def lines(hs, verdict):
  """What edits_main.cpp prints for a call, computed from HostSimEnv `hs` behind the same call."""
  out = [str(verdict)]
  for i in range(hs.cfg.num_envs):
    out.append(f'{i} {int(hs.rec[i]["status"])} ' + ' '.join(f'{fnv(hs.buf[k][i]):016x}' for k in BUFFERS))
  return out
