"""BatchedEnv's argument checks on the device: every method that takes `out=` refuses a tensor of the wrong dtype or shape, a
non-contiguous view, a tensor that is not on the batch's device and a non-tensor -- and, where the kernels store 16 bytes at a
time, a view 4 bytes off -- with ValueError before anything is enqueued: no byte of the records, of obs, reward or done changes.
An `out` it accepts holds, bit for bit, what the same call without `out` returns on a twin.  The refusals that involve no
`out` (an env named twice, world_ids without worlds, actions of the wrong length) leave the batch as it was, too."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, T = 4, 2
ALIGNED = ('step', 'step_envs', 'step_final', 'rollout', 'rollout_envs')


@pytest.fixture(scope='module')
def env():
  from crafter_amd import BatchedEnv
  env = BatchedEnv(N, seed=7, auto_reset=True)
  env.reset()
  for t in range(3):
    env.step(_acts(env, [5, 1 + t, 2, 3]), info=False)
  return env


def _acts(env, a):
  return torch.from_numpy(np.asarray(a, np.int32)).to(env.device)


# what each method is called with beside `out` (subset calls name envs 0 and 1), and the tensors a good `out` is made of
def _like(env, name):
  obs, dev = tuple(env.obs.shape[1:]), env.device
  new = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
  if name in ('step', 'step_envs', 'step_final'):
    return [new((N,) + obs, torch.uint8), new((N,), torch.float32), new((N,), torch.uint8)]
  if name in ('rollout', 'rollout_envs'):
    n = N if name == 'rollout' else 2
    return [new((T, n) + obs, torch.uint8), new((T, n), torch.float32), new((T, n), torch.uint8)]
  if name == 'symbolic':
    ls, ss = env.symbolic_shape
    return [new((N,) + ls, torch.uint8), new((N,) + ss, torch.float32)]
  if name == 'legal_actions':
    return [new((N, env.num_actions), torch.uint8)]
  return [new((N,), torch.int32)]   # level_ids


def _call(env, name, out, idx=(0, 1)):
  """The method `name` with out's tensors (None: without `out`) -> the tensors it returns, in out's order."""
  single = name in ('legal_actions', 'level_ids')
  out = None if out is None else out[0] if single else tuple(out)
  step_acts, roll_acts = [3, 5, 3, 5], [[3, 5, 3, 5], [5, 2, 5, 2]]
  if name == 'step':
    return env.step(_acts(env, step_acts), info=False, out=out)[:3]
  if name == 'step_final':
    return env.step(_acts(env, step_acts), info=False, out=out, final=True)[:3]
  if name == 'step_envs':
    return env.step_envs(list(idx), _acts(env, step_acts[:2]), info=False, out=out)[:3]
  if name == 'rollout':
    return env.rollout(_acts(env, roll_acts), out=out)
  if name == 'rollout_envs':
    return env.rollout_envs(list(idx), _acts(env, roll_acts)[:, :2], out=out)
  r = getattr(env, name)(out=out)
  return (r,) if single else r


def _bad(good, aligned):
  """good: a tensor `out` accepts -> [(what is wrong, something of its dtype and shape but for that)]"""
  shape, dt, dev = tuple(good.shape), good.dtype, good.device
  wide = torch.zeros(shape[:-1] + (2 * shape[-1],), dtype=dt, device=dev)
  cases = [('dtype', torch.zeros(shape, dtype=torch.int16, device=dev)),
           ('shape', torch.zeros(shape[:-1] + (shape[-1] + 1,), dtype=dt, device=dev)),
           ('view', wide[..., ::2]),
           ('cpu', torch.zeros(shape, dtype=dt)),
           ('non-tensor', np.zeros(shape, np.uint8))]
  if aligned:
    nbytes = good.numel() * good.element_size()
    raw = torch.zeros(nbytes + 16, dtype=torch.uint8, device=dev)
    cases.append(('4 bytes off', raw[4:4 + nbytes].view(dt).reshape(shape)))
    assert cases[-1][1].data_ptr() % 16 == 4 and cases[-1][1].is_contiguous()
  assert tuple(cases[2][1].shape) == shape and not cases[2][1].is_contiguous()
  return cases


def _frozen(env):
  return [t.clone() for t in (env.state['rec'], env.obs, env.reward, env.done)]


def _assert_frozen(env, before, what):
  for name, a, b in zip(('rec', 'obs', 'reward', 'done'), before, (env.state['rec'], env.obs, env.reward, env.done)):
    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), (what, name)


METHODS = ('step', 'step_envs', 'step_final', 'rollout', 'rollout_envs', 'symbolic', 'legal_actions', 'level_ids')


@pytest.mark.parametrize('name', METHODS)
def test_a_bad_out_is_refused_before_anything_is_enqueued(env, name):
  before = _frozen(env)
  good = _like(env, name)
  for k in range(len(good)):
    for what, bad in _bad(good[k], name in ALIGNED):
      out = list(good)
      out[k] = bad
      with pytest.raises(ValueError):
        _call(env, name, out)
      _assert_frozen(env, before, (name, k, what))
  env.check_errors()


def _same(a, b, what):
  for k, (x, y) in enumerate(zip(a, b)):
    assert x.dtype == y.dtype and torch.equal(x.view(torch.uint8), y.view(torch.uint8)), (what, k)


@pytest.mark.parametrize('name', ('step', 'step_final', 'rollout'))
def test_a_whole_batch_call_writes_into_out_what_it_returns_without(env, name):
  """(copy_envs makes twins of ROWS; the twin of a whole batch is the batch itself, put back by load_state.)"""
  store = env.save_state()
  out = _like(env, name)
  got = _call(env, name, out)
  assert all(g is o for g, o in zip(got, out))
  rec = env.state['rec'].clone()
  final = {k: v.clone() for k, v in env.final_buffers().items()} if name == 'step_final' else {}
  env.load_state(store)
  _same(out, _call(env, name, None), name)
  assert torch.equal(rec, env.state['rec'])
  _same(final.values(), [env.final_buffers()[k] for k in final], name + ' final buffers')
  env.check_errors()


@pytest.mark.parametrize('name', ('step_envs', 'rollout_envs'))
def test_a_subset_call_writes_into_out_what_its_copy_envs_twin_returns_without(env, name):
  env.copy_envs([0, 1], [2, 3])
  out = _like(env, name)
  got = _call(env, name, out, idx=(0, 1))
  assert all(g is o for g, o in zip(got, out))
  twin = _call(env, name, None, idx=(2, 3))
  if name == 'step_envs':   # full-width rows: the call with `out` wrote rows 0 and 1 of out, its twin rows 2 and 3 of the batch's own
    out, twin = [t[0:2] for t in out], [t[2:4] for t in twin]
  _same(out, twin, name)
  rec = env.state['rec']
  assert torch.equal(rec[0:2], rec[2:4])
  env.check_errors()


@pytest.mark.parametrize('name', ('symbolic', 'legal_actions', 'level_ids'))
def test_a_read_only_call_writes_into_out_what_it_returns_without(env, name):
  if name == 'level_ids':
    env.set_levels([11, 12, 13])
  out = _like(env, name)
  for t in out:
    t.fill_(77)
  got = _call(env, name, out)
  assert all(g is o for g, o in zip(got, out))
  _same(out, _call(env, name, None), name)
  if name == 'level_ids':
    assert int(out[0].min()) >= 0
    env.set_levels(None)
  env.check_errors()


def test_refusals_without_out_leave_the_batch_as_it_was(env):
  store = env.save_state([0, 1])
  before = _frozen(env)
  roll = _acts(env, [[1, 2], [3, 4]])
  for what, call in (('step_envs twice', lambda: env.step_envs([1, 1], _acts(env, [0, 0]))),
                     ('rollout_envs twice', lambda: env.rollout_envs([1, 1], roll)),
                     ('copy_envs dst twice', lambda: env.copy_envs([0, 1], [2, 2])),
                     ('load_state twice', lambda: env.load_state(store, idx=[1, 1])),
                     ('world_ids without worlds', lambda: env.reset(world_ids=[0, 0, 0, 0])),
                     ('step_envs actions', lambda: env.step_envs([0, 1], _acts(env, [0, 0, 0])))):
    with pytest.raises(ValueError):
      call()
    _assert_frozen(env, before, what)
  env.check_errors()
