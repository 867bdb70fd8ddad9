"""The rule-branch atlas (tests/atlas_cases.py) on every step path of the device: one env per case, reset into the bank
(BatchedEnv.reset(worlds=...)), each case's scripted tape against its oracle run -- pixels where drawn, reward and done at every
step, the whole state at every step (where a launch ends, for the rollouts), check_errors() at the end -- through step() on the
wide, fused, early and split kernels, without frames, with info['semantic'], with uploaded rules, on the small and the 256 x 256
geometries, and through rollout(), step_envs() and rollout_envs().  Every witness is asserted on the oracle run first
(atlas_cases.runs); the oracle runs are pinned to the reference on the CPU (tests/test_atlas_golden.py)."""
import numpy as np
import pytest
import torch

from tests import atlas_cases as ac

pytestmark = pytest.mark.gpu

I111, I110, I100, I021, I000 = ('crafter_step_kernel<%s>' % s for s in ('1, 1, 1', '1, 1, 0', '1, 0, 0', '0, 2, 1', '0, 0, 0'))
# name: (geometry, BatchedEnv arguments, environment, mutated rules, the step instance)
STEP = {
    'wide': ('default', {}, {}, False, I111),
    'fused': ('default', {}, {'CRAFTER_STEP_WIDE': '0'}, False, I111),
    'early': ('default', {}, {'CRAFTER_STEP_EARLY': '1', 'CRAFTER_STEP_WIDE': '0'}, False, I111),
    'split': ('default', {}, {'CRAFTER_SPLIT': '1'}, False, I111),
    'no-frames': ('default', dict(render=False), {}, False, I111),
    'semantic': ('default', dict(semantic=True), {}, False, I111),
    'mutated-rules': ('default', {}, {}, True, I110),
    '48x40': ('48x40', {}, {}, False, I100),
    '256-semantic': ('256', dict(semantic=True), {}, False, I021),
    '256-generic': ('256-generic', {}, {}, False, I000),
}
SHAPES = {'default': I111, '256': I021}


def _dev(a, env):
  return torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(env.device)


def _make(geometry, mutated=False, instance=None, **kw):
  """A batch of one env per case, reset into the atlas; the reset compared."""
  from crafter_amd import BatchedEnv
  g = ac.GEOMETRIES[geometry]
  rs = ac.runs(geometry, mutated)
  if mutated:
    kw['rules'] = ac.MUTATED_RULES
  env = BatchedEnv(ac.N, seeds=ac.SEEDS, auto_reset=False, **g, **kw)
  assert env.step_instance == instance
  assert env.slot_map_derived == (g['area'][0] < 256)
  obs = env.reset(worlds=ac.bank_of(env, g['area'])).cpu().numpy()
  ac.assert_step(rs, 0, obs if env.cfg.render_obs else None, snapshot=env.snapshot, where='reset: ')
  return env, rs


@pytest.mark.parametrize('name', list(STEP))
def test_atlas_step(name, monkeypatch):
  geometry, kw, environ, mutated, instance = STEP[name]
  for k, v in environ.items():
    monkeypatch.setenv(k, v)
  env, rs = _make(geometry, mutated, instance, **kw)
  tapes = ac.tapes()
  for t in range(1, ac.T + 1):
    obs, rew, done, info = env.step(_dev(tapes[t - 1], env))
    sem = info['semantic'].cpu().numpy() if kw.get('semantic') else None
    ac.assert_step(rs, t, obs.cpu().numpy() if env.cfg.render_obs else None, rew.cpu().numpy(), done.cpu().numpy(), env.snapshot, sem,
                   where=name + ': ')
  assert env.step_instance == instance
  env.check_errors()


@pytest.mark.parametrize('geometry', list(SHAPES))
@pytest.mark.parametrize('cut', [None, 13], ids=['one-call', 'two-calls'])
def test_atlas_rollout(geometry, cut):
  """rollout() of the whole tape in one call, and in two calls cut at step 13: in the middle of the scripted part of most cases."""
  env, rs = _make(geometry, instance=SHAPES[geometry])
  tapes, t0 = ac.tapes(), 0
  for end in ([ac.T] if cut is None else [cut, ac.T]):
    obs, rew, done = (x.cpu().numpy() for x in env.rollout(_dev(tapes[t0:end], env)))
    for t in range(t0 + 1, end + 1):
      ac.assert_step(rs, t, obs[t - t0 - 1], rew[t - t0 - 1], done[t - t0 - 1], where=f'rollout to {end}: ')
    ac.assert_step(rs, end, snapshot=env.snapshot, where=f'rollout to {end}: ')
    t0 = end
  assert len(ac.alive(rs, ac.T)) >= 8 and (cut is None or len(ac.alive(rs, cut)) >= 14)
  env.check_errors()


@pytest.mark.parametrize('geometry', list(SHAPES))
def test_atlas_step_envs(geometry):
  """step_envs(): every step through a freshly shuffled device list that names every case."""
  env, rs = _make(geometry, instance=SHAPES[geometry])
  tapes, rng = ac.tapes(), np.random.RandomState(5)
  for t in range(1, ac.T + 1):
    idx = rng.permutation(ac.N)
    obs, rew, done, _ = env.step_envs(_dev(idx, env), _dev(tapes[t - 1][idx], env), info=False)
    ac.assert_step(rs, t, obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy(), env.snapshot, where='step_envs: ')
  env.check_errors()


@pytest.mark.parametrize('geometry', list(SHAPES))
def test_atlas_rollout_envs(geometry):
  """rollout_envs(): two calls (cut at step 13) over shuffled lists that name every case; compact rows."""
  env, rs = _make(geometry, instance=SHAPES[geometry])
  tapes, rng, t0 = ac.tapes(), np.random.RandomState(6), 0
  for end in (13, ac.T):
    idx = rng.permutation(ac.N)
    cols = {int(i): j for j, i in enumerate(idx)}
    obs, rew, done = (x.cpu().numpy() for x in env.rollout_envs(_dev(idx, env), _dev(tapes[t0:end][:, idx], env)))
    for t in range(t0 + 1, end + 1):
      ac.assert_step(rs, t, obs[t - t0 - 1], rew[t - t0 - 1], done[t - t0 - 1], where=f'rollout_envs to {end}: ', cols=cols)
    ac.assert_step(rs, end, snapshot=env.snapshot, where=f'rollout_envs to {end}: ')
    t0 = end
  env.check_errors()
