"""-m gpu: BatchedEnv.step(final=True) (crafter_step_final): the finished episodes' last frame, terminated and the terminal
state's symbolic pair against the oracle on the workload of tests/final_ref.py (day and night deaths, asleep, truncation at the
time limit), everything else against the oracle and against the plain step path, through every step kernel and both ways to the
next world (pool, inline)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import final_ref as fr
from tests.parity import sha8

pytestmark = pytest.mark.gpu

PATTERN, STATS_PATTERN = 0xA5, -7.0


def _batched(*a, **k):
  from crafter_amd import BatchedEnv
  return BatchedEnv(*a, **k)


def _tapes(seeds, steps):
  return np.stack([fr.tape(s, steps) for s in seeds], axis=1)


def _fill(bufs):
  for k, v in bufs.items():
    v.fill_(STATS_PATTERN if v.dtype == torch.float32 else PATTERN)


def play_final(env, acts):
  """reset, then acts [T, N] through step(final=True) with the four buffers filled with a pattern before every step ->
  host arrays [T, N, ...] of obs / reward / done and of the buffers as each step left them."""
  T, n = acts.shape
  a = torch.from_numpy(acts).to(env.device)
  bufs = env.final_buffers()
  keep = {k: torch.empty((T,) + tuple(v.shape), dtype=v.dtype, device=env.device) for k, v in bufs.items()}
  obs_all = torch.empty((T,) + tuple(env.obs.shape), dtype=torch.uint8, device=env.device)
  rew_all = torch.empty((T, n), dtype=torch.float32, device=env.device)
  done_all = torch.empty((T, n), dtype=torch.uint8, device=env.device)
  env.reset()
  for t in range(T):
    _fill(bufs)
    obs, reward, done, info = env.step(a[t], info=False, final=True)
    assert set(info) == set(bufs) and all(info[k] is bufs[k] for k in bufs)
    obs_all[t], rew_all[t], done_all[t] = obs, reward, done
    for k, v in bufs.items():
      keep[k][t] = v
  env.check_errors()
  out = {k: v.cpu().numpy() for k, v in keep.items()}
  out.update(obs=obs_all.cpu().numpy(), reward=rew_all.cpu().numpy(), done=done_all.cpu().numpy())
  return out


def check_against_oracle(out, runs, fin, render=True):
  """(a) and (c): every step's obs / reward / done, every finished episode's four rows, every other row untouched."""
  T, n = out['done'].shape
  assert ('final_obs' in out) == render
  finished = 0
  for i, (run, f) in enumerate(zip(runs, fin)):
    nth = 0
    for t in range(T):
      assert bool(out['done'][t, i]) == run['done'][t] and out['reward'][t, i] == run['reward'][t], (i, t)
      if render:
        assert sha8(out['obs'][t, i]) == run['obs_sha'][t], f'obs of env {i} step {t}'
      if out['done'][t, i]:
        x = f[nth]
        nth += 1
        assert x['t'] == t
        if render:
          assert sha8(out['final_obs'][t, i]) == x['sha'], f'final_obs of env {i} step {t} (daylight {x["daylight"]:.2f}, asleep {x["sleeping"]})'
        assert out['terminated'][t, i] == int(x['terminated']), (i, t)
        assert np.array_equal(out['final_local'][t, i], x['local']), (i, t)
        assert np.array_equal(out['final_stats'][t, i].view(np.uint32), x['stats'].view(np.uint32)), (i, t, out['final_stats'][t, i], x['stats'])
      else:
        assert out['terminated'][t, i] == PATTERN and (out['final_local'][t, i] == PATTERN).all(), (i, t)
        assert (out['final_stats'][t, i] == STATS_PATTERN).all() and (not render or (out['final_obs'][t, i] == PATTERN).all()), (i, t)
    assert nth == len(f)
    finished += nth
  return finished


def _workload():
  runs, fin = fr.reference()
  fr.assert_cases(fr.SEEDS, fin)
  return runs, fin, _tapes(fr.SEEDS, fr.STEPS)


PATHS = {
    'inline': (dict(gen_period=-1), {}),
    'pool': ({}, {}),
    'fused': ({}, {'CRAFTER_STEP_WIDE': '0', 'CRAFTER_STEP_EARLY': '0'}),
    'split': ({}, {'CRAFTER_SPLIT': '1'}),
    'early': ({}, {'CRAFTER_STEP_EARLY': '1', 'CRAFTER_STEP_WIDE': '0'}),
    'wide': ({}, {'CRAFTER_STEP_WIDE': '1'}),
    'render off': (dict(render=False), {}),
    'semantic': (dict(semantic=True), {}),
}


@pytest.mark.parametrize('path', list(PATHS))
def test_final_rows_equal_the_oracle(path, monkeypatch):
  kw, env_vars = PATHS[path]
  for k, v in env_vars.items():
    monkeypatch.setenv(k, v)
  runs, fin, acts = _workload()
  env = _batched(len(fr.SEEDS), seeds=list(fr.SEEDS), length=fr.LENGTH, auto_reset=True, **kw)
  out = play_final(env, acts)
  finished = check_against_oracle(out, runs, fin, render=kw.get('render', True))
  assert finished >= len(fr.SEEDS)
  ps = env.pool_status()
  if 'gen_period' in kw:
    assert ps['state'] == 'off'
  else:   # the finished envs' next worlds came from the pool (and equal the oracle's: the frames above)
    assert ps['state'] == 'running' and ps['adopted'] > 0 and ps['adopted'] + ps['regenerated_inline'] == finished, ps


def test_final_rows_large_world():
  """area (144, 144): maps and slot table in global memory (crafter_step_kernel<0, 2, 1>); four envs, each finishes twice."""
  seeds, steps, kw = (100, 101, 102, 103), 45, dict(area=(144, 144), length=20)
  runs, fin = fr.reference(seeds, steps, tuple(sorted(kw.items())))
  assert all(len(f) == 2 for f in fin)
  for extra in (dict(gen_period=-1), {}):
    env = _batched(len(seeds), seeds=list(seeds), auto_reset=True, **kw, **extra)
    assert not env.slot_map_derived and env.step_instance == 'crafter_step_kernel<0, 2, 1>'
    assert check_against_oracle(play_final(env, _tapes(seeds, steps)), runs, fin) == 8


def _same_state(a, b, what):
  for name in ('rec', 'mat', 'mt', 'chunk_order', 'chunk_seen', 'census', 'terminal', 'semantic'):
    assert torch.equal(a.state[name], b.state[name]), (what, name)
  assert torch.equal(a.obs, b.obs) and torch.equal(a.reward, b.reward) and torch.equal(a.done, b.done), what
  # the slot tables up to each env's count (behind it: slots of worlds gone by)
  nobj = a.state['rec'].view(torch.int32)[:, a._off['nobj']]
  live = torch.arange(a.cfg.max_objects, device=a.device)[None, :] < nobj[:, None]
  assert torch.equal(a.state['objs'][live], b.state['objs'][live]), (what, 'objs')


@pytest.mark.parametrize('gen_period', [0, -1], ids=['pool', 'inline'])
def test_final_path_is_the_plain_path(gen_period):
  """(b) two batches, same seeds and actions, one with final=True: obs, reward, done, terminal, info['semantic'], records() and
  snapshot(i) after every step; then 30 more steps with the modes swapped."""
  seeds = list(fr.SEEDS)
  acts = torch.from_numpy(_tapes(fr.SEEDS, fr.STEPS + 30)).cuda()
  kw = dict(seeds=seeds, length=fr.LENGTH, auto_reset=True, semantic=True, gen_period=gen_period)
  a, b = _batched(len(seeds), **kw), _batched(len(seeds), **kw)
  a.reset(), b.reset()
  episodes = 0
  for t in range(fr.STEPS + 30):
    swapped = t >= fr.STEPS
    _, _, _, ia = a.step(acts[t], final=swapped)
    _, _, _, ib = b.step(acts[t], final=not swapped)
    assert ('terminated' in ia) == swapped and ('terminated' in ib) == (not swapped)
    assert torch.equal(ia['semantic'], ib['semantic']), t
    _same_state(a, b, t)
    done = a.done.cpu().numpy().astype(bool)
    if done.any() or t % 25 == 0:   # ... and literally, on the host, wherever an env was handed on
      ra, rb = a.records(), b.records()
      assert ra.tobytes() == rb.tobytes(), t
      for i in (np.flatnonzero(done) if done.any() else [0]):
        sa, sb = a.snapshot(int(i)), b.snapshot(int(i))
        assert sa.keys() == sb.keys()
        for k in sa:
          assert np.array_equal(sa[k], sb[k]) if isinstance(sa[k], np.ndarray) else sa[k] == sb[k], (t, i, k)
      episodes += int(done.sum())
  assert episodes >= len(seeds)
  a.check_errors(), b.check_errors()
  if gen_period == 0:
    pa, pb = a.pool_status(), b.pool_status()
    assert (pa['adopted'], pa['regenerated_inline']) == (pb['adopted'], pb['regenerated_inline']) and pa['adopted'] > 0


def test_errors():
  """(e) final=True without auto_reset raises; the C call on such a handle returns non-zero with a text."""
  from crafter_amd import lib as hiplib
  env = _batched(2, seeds=[1, 2], auto_reset=False)
  env.reset()
  acts = torch.zeros(2, dtype=torch.int32, device=env.device)
  with pytest.raises(ValueError, match='auto_reset'):
    env.step(acts, final=True)
  term = torch.zeros(2, dtype=torch.uint8, device=env.device)
  p = lambda t: C.c_void_p(t.data_ptr())
  rc = env._lib.crafter_step_final(env._handle, p(acts), p(env.obs), p(env.reward), p(env.done), None, p(term), None, None, env._stream())
  assert rc != 0 and 'auto_reset' in hiplib.last_error(env._lib, env._handle)
  on = _batched(2, seeds=[1, 2], auto_reset=True)
  on.reset()
  rc = on._lib.crafter_step_final(on._handle, p(acts), p(on.obs), p(on.reward), p(on.done), None, None, None, None, on._stream())
  assert rc != 0 and 'null' in hiplib.last_error(on._lib, on._handle)
  obs, reward, done, info = on.step(acts, info=False)   # the default: today's return value
  assert info == {}


def test_vec_env_view_with_auto_reset():
  """(f) VecEnvView(auto_reset=True) against VecEnvView(): obs / reward / done, terminal_observation, TimeLimit.truncated -- and
  the finished episodes' inventory, achievements and discount, which the new mode takes from final_stats / terminal / terminated."""
  from crafter_amd.vec import VecEnvView
  seeds = [111, 101, 108, 104]
  acts = _tapes(seeds, fr.STEPS)
  a = VecEnvView(len(seeds), seeds=seeds, length=fr.LENGTH, auto_reset=True)
  b = VecEnvView(len(seeds), seeds=seeds, length=fr.LENGTH)
  assert np.array_equal(a.reset(), b.reset())
  ends, truncated = 0, 0
  for t in range(fr.STEPS):
    oa, ra, da, ia = a.step(acts[t])
    ob, rb, db, ib = b.step(acts[t])
    assert np.array_equal(oa, ob) and np.array_equal(ra, rb) and np.array_equal(da, db), t
    for i in range(len(seeds)):
      assert ('terminal_observation' in ia[i]) == bool(da[i]) == ('terminal_observation' in ib[i])
      if da[i]:
        assert np.array_equal(ia[i]['terminal_observation'], ib[i]['terminal_observation']), (t, i)
        assert ia[i]['TimeLimit.truncated'] == ib[i]['TimeLimit.truncated']
        assert ia[i]['inventory'] == ib[i]['inventory'] and ia[i]['achievements'] == ib[i]['achievements']
        assert ia[i]['discount'] == ib[i]['discount'] and abs(ia[i]['reward'] - ib[i]['reward']) < 1e-6
        ends += 1
        truncated += int(ia[i]['TimeLimit.truncated'])
  assert ends >= 4 and 1 <= truncated < ends
