"""The rule-branch atlas (tests/atlas_cases.py) on the CPU harness of the kernel bodies: every case, reset through
crafter_reset_worlds' body, against its oracle run -- pixels, reward, done and the whole state at every step -- on every
object-lookup layout and rule-table mode the device has (the cell -> slot map in LDS, LaneSlots of the split rules kernel, FarSlot
of the 256 x 256 worlds with the product's and with a 3-entry cache, compiled-in and uploaded rules) and through the rollout,
subset and subset-rollout bodies.  The oracle runs are pinned to the reference by tests/test_atlas_golden.py."""
import numpy as np
import pytest

from tests import atlas_cases as ac
from tests.hostsim import worlds_build
from tests.hostsim.driver import HostSimEnv, lib

TINY = ('fartiny', ('CRAFTER_FAR_CACHE=3', 'CRAFTER_FAR_HOLES=2'))   # tests/test_large_world.py: nearly every record misses the cache
# name: (geometry, HostSimEnv arguments, split mode, mutated rules).  The harness passes split 0 / 1 to choose_step, never the
# device's "unset", so a build without frames reaches LaneSlots only with split = 1 (with 0: the slot-map body, no frame)
BUILDS = {
    'default': ('default', dict(want_semantic=True), 0, False),
    'split-lane-slots': ('default', dict(want_semantic=True), 1, False),
    'no-frames-lane-slots': ('default', dict(render_obs=False), 1, False),   # the rules kernel's body alone: what render=False runs
    '48x40': ('48x40', {}, 0, False),
    '256-far-slot': ('256', dict(want_semantic=True), 0, False),
    '256-far-cache-3': ('256', dict(variant=TINY), 0, False),
    '256-generic': ('256-generic', {}, 0, False),
    'mutated-rules': ('default', {}, 0, True),
}


def make(geometry, mutated=False, **kw):
  """A HostSimEnv of one env per case, reset into the atlas; the reset itself compared."""
  g = ac.GEOMETRIES[geometry]
  rules = ac.MUTATED_RULES if mutated else None
  hs = HostSimEnv(ac.SEEDS, auto_reset=False, rules=rules, **g, **kw)
  assert worlds_build.reset_worlds(hs, ac.bank_of(hs, g['area'])) == 0
  return hs


def semantic_of(hs):
  return hs.buf['semantic'] if hs.cfg.want_semantic else None


@pytest.mark.parametrize('name', list(BUILDS))
def test_atlas_step_by_step(name):
  geometry, kw, split, mutated = BUILDS[name]
  rs = ac.runs(geometry, mutated)
  l = lib(kw.get('variant'))
  l.hostsim_set_split(split)
  try:
    hs = make(geometry, mutated, **kw)
    frames = hs.cfg.render_obs
    ac.assert_step(rs, 0, hs.obs if frames else None, snapshot=hs.snapshot, semantic=semantic_of(hs), where=name + ': ')
    tapes = ac.tapes()
    for t in range(1, ac.T + 1):
      obs, rew, done = hs.step(tapes[t - 1])
      ac.assert_step(rs, t, obs if frames else None, rew, done, hs.snapshot, semantic_of(hs), where=name + ': ')
  finally:
    l.hostsim_set_split(0)
  assert not hs.rec['status'].any()


@pytest.mark.parametrize('geometry', ['default', '256'])
@pytest.mark.parametrize('cut', [None, 13], ids=['one-call', 'two-calls'])
def test_atlas_rollout(geometry, cut):
  """crafter_step_n's body: the whole tape in one call, and in two calls cut at step 13 -- in the middle of the scripted part of
  most cases.  Every step's outputs; the state where a call ends."""
  rs = ac.runs(geometry)
  hs = make(geometry)
  tapes, t0 = ac.tapes(), 0
  for end in ([ac.T] if cut is None else [cut, ac.T]):
    obs, rew, done = hs.step_n(tapes[t0:end])
    for t in range(t0 + 1, end + 1):
      ac.assert_step(rs, t, obs[t - t0 - 1], rew[t - t0 - 1], done[t - t0 - 1], where=f'rollout to {end}: ')
    ac.assert_step(rs, end, snapshot=hs.snapshot, where=f'rollout to {end}: ')
    t0 = end
  assert len(ac.alive(rs, ac.T)) >= 8 and (cut is None or len(ac.alive(rs, cut)) >= 14)
  assert not hs.rec['status'].any()


@pytest.mark.parametrize('geometry', ['default', '256'])
def test_atlas_step_envs(geometry):
  """crafter_step_envs' body: every step through a freshly shuffled list that names every case."""
  from tests.hostsim import subset_build as sb
  rs = ac.runs(geometry)
  hs = make(geometry)
  marks, tapes, rng = sb.Marks(ac.N), ac.tapes(), np.random.RandomState(5)
  for t in range(1, ac.T + 1):
    idx = rng.permutation(ac.N)
    assert sb.step_envs(hs, marks, idx, tapes[t - 1][idx]) == 0
    ac.assert_step(rs, t, hs.obs, hs.reward, hs.done, hs.snapshot, where='step_envs: ')
  assert not hs.rec['status'].any()


@pytest.mark.parametrize('geometry', ['default', '256'])
def test_atlas_rollout_envs(geometry):
  """crafter_step_n_envs' body: two calls (cut at step 13) over shuffled lists that name every case, compact rows."""
  from tests.hostsim import rollout_envs_build as rb
  rs = ac.runs(geometry)
  hs = make(geometry)
  marks, tapes, rng, t0 = rb.Marks(ac.N), ac.tapes(), np.random.RandomState(6), 0
  for end in (13, ac.T):
    idx = rng.permutation(ac.N)
    cols = {int(i): j for j, i in enumerate(idx)}
    verdict, obs, rew, done = rb.rollout_envs(hs, marks, idx, tapes[t0:end][:, idx])
    assert verdict == 0
    for t in range(t0 + 1, end + 1):
      ac.assert_step(rs, t, obs[t - t0 - 1], rew[t - t0 - 1], done[t - t0 - 1], where=f'rollout_envs to {end}: ', cols=cols)
    ac.assert_step(rs, end, snapshot=hs.snapshot, where=f'rollout_envs to {end}: ')
    t0 = end
  assert not hs.rec['status'].any()
