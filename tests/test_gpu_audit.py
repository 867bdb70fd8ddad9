"""-m gpu: BatchedEnv.audit() -- crafter_audit through the C ABI -- stays silent on every path that writes rows (step, step_envs,
rollout, rollout_envs, copy_envs, save_state / load_state, edit, reset(worlds=...), set_levels, step(final=True), adoptions of
pooled worlds, 256 x 256 worlds after every step), equals the numpy mirror on flags and detail, names each corruption of
tests/audit_cases.py, and audits a 1024-env soak after every step.  A corrupted row is only ever handed to the audit: it is
restored from a store before the batch is stepped again."""
import numpy as np
import pytest
import torch

from crafter_amd import abi, state
from tests import audit_cases as cases

pytestmark = pytest.mark.gpu

LENGTH = 200   # an episode ends in its first night (daylight < 0.5 from step 148 on)


def _batched(*a, **k):
  from crafter_amd import BatchedEnv
  return BatchedEnv(*a, **k)


def _dev(a, env, dtype=np.int32):
  return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(env.device)


def _names(bits):
  return [n for b, n in enumerate(abi.AUDIT_NAMES) if bits >> b & 1]


def _assert_clean(env, where):
  flags, detail = env.audit()
  f = flags.cpu().numpy()
  bad = np.nonzero(f)[0]
  assert not len(bad), f'{where}: env {bad[0]} fails {_names(int(f[bad[0]]))}, detail {detail[bad[0]].tolist()}'
  assert bool((detail == -1).all()), where


@pytest.mark.parametrize('geo', [dict(area=(64, 64)), dict(area=(42, 30), view=(7, 9), size=(84, 72))], ids=['64x64', '42x30'])
def test_clean_on_every_path(geo):
  """16 envs, pool on, 320 steps through a night and the auto-resets behind it, the calls dealt in turn to every entry point
  that writes rows; after each call every row is a row."""
  from crafter_amd import WorldBank, edits as E
  from tests import edits_cases as ec, worlds_cases as wc
  n = 16
  env = _batched(n, seeds=[300 + i for i in range(n)], auto_reset=True, length=LENGTH, **geo)
  assert env.slot_map_derived and env.pool_status(stats=False)['state'] == 'running'
  flags, detail = env.audit()
  assert bool((flags == abi.AUDIT_NOT_RESET).all()) and detail.cpu().tolist() == [[0, -1, -1, -1]] * n
  env.reset()
  _assert_clean(env, 'reset')
  rs = np.random.RandomState(4)
  daylight = np.asarray(env.tables.daylight)
  acts = lambda *shape: _dev(rs.randint(0, 17, shape), env)
  step_of = lambda: state.rec_view(env.state['rec'].cpu().numpy())['step'].copy()
  world = wc.small_world(geo['area'])
  bank = WorldBank(env, world['mat'][None], [world['objects']], [world['inventory']])
  night = balance = episodes = t = call = 0
  store = None
  while t < 320:
    kind = call % 10
    call += 1
    before, steps, done = step_of(), 1, None
    if kind in (0, 5):
      done = env.step(acts(n), info=False)[2]
    elif kind == 1:
      idx = rs.permutation(n)
      for half in (idx[:7], idx[7:]):
        episodes += int(env.step_envs(_dev(half, env), acts(len(half)), info=False)[2][_dev(half, env, np.int64)].sum())
        _assert_clean(env, f'call {call}: step_envs')
    elif kind == 2:
      steps = 4
      done = env.rollout(acts(steps, n), obs=False)[2]
    elif kind == 3:
      steps = 3
      idx = rs.permutation(n)
      for half in (idx[:5], idx[5:]):
        episodes += int(env.rollout_envs(_dev(half, env), acts(steps, len(half)), obs=False)[2].sum())
        _assert_clean(env, f'call {call}: rollout_envs')
    elif kind == 4:
      env.copy_envs([0, 1], [14, 15])
      _assert_clean(env, f'call {call}: copy_envs')
      done = env.step(acts(n), info=False)[2]
    elif kind == 6:
      if store is None:
        store = env.save_state([2, 3, 4])
      else:
        env.load_state(store, idx=[5, 6, 7])
        store = None
      _assert_clean(env, f'call {call}: save_state / load_state')
      done = env.step(acts(n), info=False)[2]
    elif kind == 7:
      mask = np.zeros(n, np.uint8)
      mask[[8, 9]] = 1
      env.reset(mask=_dev(mask, env, np.uint8), worlds=bank)
      _assert_clean(env, f'call {call}: reset(worlds=)')
      env.edit([9, 8], ec.geometry_edits(geo['area'])[0])   # (a tape written for this world right behind its reset)
      _assert_clean(env, f'call {call}: edit')
      env.edit([0, 1, 2], [E.set_cell(3, 3, 'path'), E.set_cell(4, 3, 'grass'), E.set_item('wood', 2), E.set_player(hunger2=10)])
      _assert_clean(env, f'call {call}: edit of any row')
      done = env.step(acts(n), info=False)[2]
    elif kind == 8:
      if call == 9:     # (early in the run only: a new table empties the pool, and the night's auto-resets are to adopt from it)
        env.set_levels([11, 12, 13], weights=[1, 2, 1])
      elif call == 19:
        env.set_levels(None)
      _assert_clean(env, f'call {call}: set_levels')
      done = env.step(acts(n), info=False)[2]
    else:
      done = env.step(acts(n), final=True)[2]
    if done is not None:
      episodes += int(done.sum())
    t += steps
    _assert_clean(env, f'call {call} kind {kind} at step {t}')
    for a, z in zip(before, step_of()):   # the steps an env played in this call (none counted across a reset)
      played = np.arange(a + 1, z + 1)
      night += int((daylight[played] < 0.5).sum())
      balance += int(((daylight[played] < 0.5) & (played % 10 == 0)).sum())
  assert night >= 100 and balance >= 8 and episodes >= 4, (night, balance, episodes)
  assert env.pool_status()['adopted'] > 0
  env.assert_consistent()
  env.check_errors()


def test_clean_256x256_every_step():
  """The seeds and tapes of test_config4_tables_in_global_memory_stay_consistent (deaths, adoptions of pooled worlds, the evening's
  balance passes), the whole audit -- slot map, census, chunk tables -- after every step of 260, one word read back per step."""
  seeds = [42, 43, 49, 51, 40, 45, 46, 55]
  T = 260
  tapes = np.stack([np.random.RandomState(900 + s).choice([0, 0, 0, 1, 2, 3, 4, 5, 6], size=T) if s % 2 == 0 else
                    np.random.RandomState(900 + s).randint(0, 17, size=T) for s in seeds], 1).astype(np.int32)
  env = _batched(len(seeds), area=(256, 256), seeds=seeds, auto_reset=True)
  assert not env.slot_map_derived
  env.reset()
  dev = torch.from_numpy(tapes).to(env.device)
  out = torch.zeros(len(seeds), dtype=torch.int32, device=env.device), torch.zeros((len(seeds), 4), dtype=torch.int32, device=env.device)
  episodes = 0
  for t in range(T):
    _, _, done, _ = env.step(dev[t], info=False)
    flags, detail = env.audit(out=out)
    word = int(flags.max())   # (flags are non-negative: the maximum is 0 iff all are)
    assert word == 0, f'step {t}: {[(i, _names(f), d) for i, (f, d) in enumerate(zip(flags.tolist(), detail.tolist())) if f]}'
    episodes += int(done.sum())
  assert episodes >= 4
  env.check_errors()


def _corruption_batch(geo):
  env = _batched(6, seeds=[900 + i for i in range(6)], auto_reset=True, **geo)
  env.reset()
  rs = np.random.RandomState(9)
  for _ in range(12):   # (the generator's zombies still stand: daylight despawns them)
    env.step(_dev(rs.randint(0, 17, 6), env), info=False)
  ctx = cases.Ctx(env.cfg, env.tables.rules, not env.slot_map_derived)
  return env, ctx


def _upload(env, buf, rows):
  """Rows `rows` of the numpy buffers -> env.state (the caller-owned tensors: a poke from outside, as the scripted-tape tests do)."""
  for k, a in buf.items():
    t = env.state[k]
    src = torch.from_numpy(np.ascontiguousarray(a[rows]).view(np.uint8).reshape(len(rows), -1))
    t.view(torch.uint8).reshape(t.shape[0], -1)[rows] = src.to(env.device)


SENTINEL = 0x3C3C3C3C


@pytest.fixture(scope='module', params=[dict(area=(64, 64)), dict(area=(256, 256))], ids=['64x64', '256x256'])
def corruption_run(request):
  """One pass over the table for the two tests below (one batch, one download per case): every case applied to rows 1 and 3
  of a batch of 6 by writing env.state, audited under a mask that leaves rows 2 and 5 out, and mirrored from the downloaded
  buffers.  Then the rows come back from a store saved before the first corruption and are audited again; only then the batch
  is stepped once and check_errors() runs.  -> {case: (device flags, detail, expected, mirror flags, detail)}; 'clean' and
  'restored' hold the batch before and behind."""
  env, ctx = _corruption_batch(request.param)
  store = env.save_state()
  clean = cases.host_buffers(env.state, ctx)
  mirror = lambda: state.audit_host({k: env.state[k] for k in clean}, env.cfg, env.tables.rules, env.slot_map_derived)
  both = lambda **kw: tuple(t.cpu().numpy() for t in env.audit(**kw))
  runs = {'clean': both() + ({},) + mirror()}
  mask = _dev([1, 1, 0, 1, 1, 0], env, np.uint8)
  names = list(cases.cases(ctx))
  assert len(names) == (25 if ctx.map_state else 22)
  for name in names:
    buf, want = cases.corrupted(clean, name, (1, 3), ctx)
    _upload(env, buf, [1, 3])
    out = torch.full((6,), SENTINEL, dtype=torch.int32, device=env.device), torch.full((6, 4), SENTINEL, dtype=torch.int32, device=env.device)
    runs[name] = both(mask=mask, out=out) + (want,) + mirror()
  env.load_state(store)
  runs['restored'] = both() + ({},) + mirror()
  assert not runs['restored'][0].any(), 'a row did not come back from the store: the batch is not stepped'
  env.step(_dev(np.zeros(6), env), info=False)
  _assert_clean(env, 'stepped')
  env.check_errors()
  return runs


def test_finds_each_corruption(corruption_run):
  """The case's bits and detail on rows 1 and 3, 0 and -1 on the other audited rows, the sentinel on the masked ones; clean
  before, clean again once restored."""
  for name, (flags, detail, want, _, _) in corruption_run.items():
    if name in ('clean', 'restored'):
      cases.check(flags, detail, {}, name)
      continue
    assert flags[2] == SENTINEL and flags[5] == SENTINEL and (detail[[2, 5]] == SENTINEL).all(), name
    cases.check(flags, detail, want, name, untouched=(2, 5))


def test_matches_host_mirror(corruption_run):
  """Device flags and detail equal crafter_amd.audit_host over the downloaded buffers: clean rows and every corrupted row."""
  for name, (flags, detail, _, mf, md) in corruption_run.items():
    keep = list(range(6)) if name in ('clean', 'restored') else [0, 1, 3, 4]
    assert np.array_equal(mf[keep], flags[keep]) and np.array_equal(md[keep], detail[keep]), (name, mf, flags, md[[1, 3]], detail[[1, 3]])


def test_single_env_and_run_random_facades(capsys):
  """Env.audit() names nothing for an env under way; run_random --audit K plays its episodes through with an audit every K steps."""
  from crafter_amd import Env, run_random
  env = Env(seed=3)
  env.reset()
  for a in (1, 5, 2, 5):
    env.step(a)
  assert env.audit() == []
  run_random.main(['--envs', '8', '--episodes', '1', '--length', '40', '--seed', '2', '--audit', '5'])
  assert 'Episodes finished:' in capsys.readouterr().out   # (it ran to its end: a finding raises CrafterDeviceError)


def test_soak_audited_every_step():
  """The worked example of the README: 1024 envs, 600 random steps, an audit after every step, the flags OR-ed on the device and
  read back once.  Then a census word made stale from outside: assert_consistent() names the row, SPACE and the chunk."""
  from crafter_amd import CrafterDeviceError
  n, T = 1024, 600
  env = _batched(n, seed=5000, auto_reset=True)
  env.reset()
  tape = torch.from_numpy(np.random.RandomState(8).randint(0, 17, size=(T, n)).astype(np.int32)).to(env.device)
  out = torch.zeros(n, dtype=torch.int32, device=env.device), torch.zeros((n, 4), dtype=torch.int32, device=env.device)
  seen = torch.zeros(n, dtype=torch.int32, device=env.device)
  for t in range(T):
    env.step(tape[t], info=False)
    seen |= env.audit(out=out)[0]
  assert int(seen.max()) == 0, [(i, _names(f)) for i, f in enumerate(seen.tolist()) if f][:4]
  env.assert_consistent()
  env.check_errors()
  row, chunk = 77, 14
  word = env.state['census'][row, chunk * 5].clone()
  env.state['census'][row, chunk * 5] += 1
  with pytest.raises(CrafterDeviceError, match=rf'env {row}: SPACE \(SPACE: index {chunk * 5} at chunk {chunk} column 0'):
    env.assert_consistent()
  env.state['census'][row, chunk * 5] = word
  env.assert_consistent()
