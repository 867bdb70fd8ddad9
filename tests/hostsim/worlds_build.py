"""TEST INFRASTRUCTURE: crafter_reset_worlds on the CPU (worlds_host.cpp, built by tests/hostsim/build.py) over a HostSimEnv's
cfg / tb / st and a crafter_amd.WorldBank; and the stand-alone program of the same code (worlds_main.cpp, built with
-fsanitize=address,undefined), which plays a dumped call."""
import ctypes as C
import struct

import numpy as np

from . import build as _build
from .build import fnv, ptr as _p


def build_sanitized():
  return _build.build('worlds_main')


def lib():
  return _build.lib('worlds')


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
  return lib().hostsim_reset_worlds(C.byref(hs.cfg), C.byref(hs.tb), C.byref(hs.st), *[_p(a) for a in arrays], n_worlds, cap, _p(hs.obs))


def dump(hs, bank, path, mask=None, world_ids=None):
  """Writes HostSimEnv `hs` (as it stands) and the call's arguments as the blob worlds_main.cpp reads."""
  arrays, n_worlds, cap = _args(hs, bank, mask, world_ids)
  _build.write_blob(path, [struct.pack('<2i', n_worlds, cap)] + _build.env_parts(hs) + [b'' if a is None else a.tobytes() for a in arrays])


def lines(hs, mask=None):
  """What worlds_main.cpp prints for a call with `mask`, computed from HostSimEnv `hs`."""
  out = []
  for i in range(hs.cfg.num_envs):
    row = [fnv(hs.buf[k][i]) for k in ('mat', 'objs', 'mt', 'rec', 'chunk_order', 'census')] + [
        0 if mask is not None and not mask[i] else fnv(hs.obs[i])]
    out.append(f'{i} {int(hs.rec[i]["status"])} ' + ' '.join(f'{v:016x}' for v in row))
  return out
