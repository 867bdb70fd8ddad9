"""TEST INFRASTRUCTURE: the three generator forms on the CPU (generator_forms_host.cpp, built by tests/hostsim/build.py) over a
HostSimEnv's cfg / tb / st -- Env.reset into the env's row, the fused form into a pool entry, the three-stage pipeline into a
pool entry -- and the stand-alone program of the same calls (generator_forms_main.cpp, built with -fsanitize=address,undefined),
which plays a dumped env."""
import ctypes as C

import numpy as np

from . import build as _build
from .build import fnv, ptr as _p

FIELDS = ('mat', 'objs', 'mt', 'mt_pos', 'chunk_order', 'census')   # what a world is, whichever form made it


def build_sanitized():
  return _build.build('generator_forms_main')


def lib():
  return _build.lib('generator_forms')


def _world(mat, objs, nobj, mt, mt_pos, order, nseen, census):
  """The canonical fields: the live prefix of the slot table and the seen prefix of the chunk order (what lies behind either is
  whatever the buffer held before)."""
  return dict(mat=mat.copy(), objs=objs[:int(nobj)].copy(), mt=mt.copy(), mt_pos=int(mt_pos), chunk_order=order[:int(nseen)].copy(),
              census=census.copy())


def reset_world(hs, env, episode):
  """Env.reset of row `env` into `episode` (reset_body, world pool off) -> the world in the row."""
  hs.rec[env]['episode'] = episode - 1
  got = lib().hostsim_forms_reset(C.byref(hs.cfg), C.byref(hs.tb), C.byref(hs.st), env, _p(hs.obs))
  assert got == episode
  r = hs.rec[env]
  return _world(hs.buf['mat'][env], hs.buf['objs'][env], r['nobj'], hs.buf['mt'][env], r['mt_pos'], hs.buf['chunk_order'][env], r['nchunks_seen'],
                hs.buf['census'][env])


def pool_world(hs, env, episode, form):
  """The world of (env, episode) generated into its pool entry by `form` ('fused': gen_body, 'pipeline': seed -> classify ->
  resolve), the entry's header emptied first -> the world in the entry."""
  e = episode & 1
  hs.pool_hdr[e, env] = 0
  call = lib().hostsim_forms_fused if form == 'fused' else lib().hostsim_forms_pipeline
  call(C.byref(hs.cfg), C.byref(hs.tb), C.byref(hs.st), env, episode)
  h = hs.pool_hdr[e, env]
  assert int(h['ready']) == (1 << 32 | episode), 'the entry was not published'
  return _world(hs.buf['pool_mat'][e, env], hs.buf['pool_objs'][e, env], h['nobj'], hs.buf['pool_mt'][e, env], h['mt_pos'],
                hs.buf['pool_chunk_order'][e, env], h['nchunks_seen'], hs.buf['pool_census'][e, env])


def dump(hs, path, pairs):
  """Writes the (env, episode) pairs and HostSimEnv `hs` (as it stands) as the blob generator_forms_main.cpp reads."""
  _build.write_blob(path, [np.asarray(pairs, np.int32).reshape(-1, 2).tobytes()] + _build.env_parts(hs))


def line(form, env, episode, w):
  """What generator_forms_main.cpp prints for world `w` (a dict of FIELDS)."""
  return (f'{form} {env} {episode} {len(w["objs"])} {w["mt_pos"]} {len(w["chunk_order"])} ' +
          ' '.join(f'{fnv(w[k]):016x}' for k in ('mat', 'objs', 'mt', 'chunk_order', 'census')))
