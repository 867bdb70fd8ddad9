"""TEST INFRASTRUCTURE: crafter_nearby's body on the CPU (nearby_host.cpp, built by tests/hostsim/build.py) over a HostSimEnv's
cfg / tb / st or over any dict of raw buffers laid out like them; and the stand-alone program of the same code (nearby_main.cpp,
built with -fsanitize=address,undefined), which reads a dumped HostSimEnv."""
import ctypes as C
import struct
import subprocess

import numpy as np

from crafter_amd import abi
from . import build as _build
from .build import ptr as _p

_build.LIBS.setdefault('nearby', 'nearby_host.cpp')
_build.PROGRAMS.setdefault('nearby_main', 'nearby_main.cpp')

BUFFERS = ('mat', 'objmap', 'objs', 'rec')   # what the body reads of a row


def build_sanitized():
  return _build.build('nearby_main')


def lib():
  l = _build.lib('nearby')
  l.hostsim_nearby_error.restype = C.c_char_p
  return l


def map_is_state(hs):
  return bool(lib().hostsim_nearby_map_is_state(C.byref(hs.cfg)))


def in_wave(hs):
  return bool(lib().hostsim_nearby_in_wave(C.byref(hs.cfg)))


def lds_bytes(hs, k):
  return int(lib().hostsim_nearby_lds_bytes(C.byref(hs.cfg), C.c_int(k)))


def n_classes(hs):
  return int(hs.tab.rules.n_materials) + 1 + abi.T_PLANT


def error_text(reason):
  return lib().hostsim_nearby_error(C.c_int(reason)).decode()


def call(hs, mask, distance, flags, classes, k, counts, ents, n, force_map=-1, walk=-1, buf=None):
  """hostsim_nearby with the arguments as given (numpy arrays or None) -> its return value.  buf: other raw buffers of the same
  shapes in the HostSimEnv's place."""
  st = hs.st
  if buf is not None:
    st = abi.StatePtrs(**{name: (_p(buf[name]).value if name in buf else None) for name, _ in abi.StatePtrs._fields_})
  return lib().hostsim_nearby(C.byref(hs.cfg), C.byref(hs.tb), C.byref(st), _p(mask), C.c_int32(distance), C.c_int32(flags), C.c_uint32(classes),
                              C.c_int32(k), _p(counts), _p(ents), _p(n), C.c_int(force_map), C.c_int(walk))


def nearby(hs, distance, k, classes, numpy_slices=False, mask=None, force_map=-1, walk=-1, buf=None):
  """hostsim_nearby over HostSimEnv `hs`: distance (None or negative: the whole world), classes (a class set as an int) ->
  (counts int32 [N, C], ents int16 [N, k, 6], n int32 [N]), masked rows holding the fill 0x7E7E.."""
  N = hs.cfg.num_envs
  counts = np.full((N, n_classes(hs)), 0x7E7E7E7E, np.int32)
  ents, n = np.full((N, k, abi.NEARBY_ROW), 0x7E7E, np.int16), np.full(N, 0x7E7E7E7E, np.int32)
  m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
  rc = call(hs, m, -1 if distance is None else distance, int(numpy_slices), classes, k, counts, ents if k else None, n if k else None,
            force_map, walk, buf)
  assert rc == 0, (rc, error_text(rc))
  return counts, ents, n


def dump(hs, path, distance, k, classes, numpy_slices=False, mask=None, walk=-1, buf=None):
  """Writes what the body reads of HostSimEnv `hs` as it stands (or `buf`) and the query as the blob nearby_main.cpp reads."""
  buf = hs.buf if buf is None else buf
  state_map = map_is_state(hs)
  parts = [bytes(hs.cfg), np.ascontiguousarray(hs._rules_buf).tobytes(), struct.pack('<i', int(state_map))]
  parts += [b'' if (name == 'objmap' and not state_map) else np.ascontiguousarray(buf[name]).tobytes() for name in BUFFERS]
  parts.append(b'' if mask is None else np.ascontiguousarray(mask, np.uint8).tobytes())
  parts.append(struct.pack('<iiIii', -1 if distance is None else distance, int(numpy_slices), classes, k, walk))
  _build.write_blob(path, parts)


def run_sanitized(path, n_cls, k):
  """-> the program's rows: per env None (row left untouched) or (counts [C], n, ents [k][6]) as lists of ints."""
  proc = subprocess.run([str(build_sanitized()), str(path)], capture_output=True, text=True)
  assert proc.returncode == 0, proc.stderr[-3000:]
  rows = []
  for line in proc.stdout.splitlines():
    if line == '-':
      rows.append(None)
      continue
    v = [int(x) for x in line.split()]
    assert len(v) == n_cls + 1 + k * abi.NEARBY_ROW
    rows.append((v[:n_cls], v[n_cls], [v[n_cls + 1 + abi.NEARBY_ROW * j: n_cls + 1 + abi.NEARBY_ROW * (j + 1)] for j in range(k)]))
  return rows
