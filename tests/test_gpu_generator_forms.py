"""-m gpu: the three ways the library makes the world of one (seed, episode) agree on the device -- the statement of
tests/test_generator_forms_host.py through the kernels themselves.
  batch A  world pool off (gen_period=-1), reset() k times: its rows hold the fused world of episode k (crafter_reset_kernel)
  batch B  world pool on, a batch after every step (gen_period=1): reset() leaves episode 2 in pool entry (2 & 1) * N + env,
           by the fused form into a pool entry (gen_body, appended by crafter_reset_kernel), and asks the pool for episode 3;
           the batch behind one noop step() writes it into entry (3 & 1) * N + env by the three generation kernels
Equal means: the material map, the live prefix of the slot table, the MT state and its position, the seen prefix of the chunk
order and the census.  No field is left out: an entry's header carries nobj, mt_pos and nchunks_seen as the row's record does."""
import numpy as np
import pytest
import torch

from crafter_amd import abi, state

pytestmark = pytest.mark.gpu

FIELDS = ('mat', 'objs', 'mt', 'mt_pos', 'chunk_order', 'census')
SHAPES = {   # n, area, view, size
    '8x64x64': (8, (64, 64), (9, 9), (64, 64)),
    '4x42x30': (4, (42, 30), (7, 9), (84, 72)),     # 1260 cells: a classification part and a 236-cell tail
    '2x256x256': (2, (256, 256), (9, 9), (64, 64)),   # maps and slot table generated in place in the pool entry
}


def _host(env, name):
  return env.state[name].cpu().numpy()


def row_worlds(env):
  """The worlds in the rows of `env`, one dict of FIELDS per env."""
  rec = state.rec_view(_host(env, 'rec'))
  mat, objs, mt, order, census = (_host(env, k) for k in ('mat', 'objs', 'mt', 'chunk_order', 'census'))
  return [dict(mat=mat[i], objs=objs[i][:rec[i]['nobj']], mt=mt[i], mt_pos=int(rec[i]['mt_pos']), chunk_order=order[i][:rec[i]['nchunks_seen']],
               census=census[i]) for i in range(env.num_envs)]


def entry_worlds(env, episode):
  """The worlds in the pool entries (episode & 1) * N + i of `env`, which must be published as holding `episode`."""
  e = episode & 1
  hdr = _host(env, 'pool_hdr').view(abi.POOL_HDR_DTYPE).reshape(2, -1)[e]
  for i, h in enumerate(hdr):
    ready = int(h['ready'])
    assert ready & 0xFFFFFFFF == episode and ready >> 32 >= 1, f'entry of env {i} does not hold episode {episode}: ready = {ready:#x}'
    assert h['pad'] == 0, f'status bits {h["pad"]:#x} came with the world of env {i}'
  mat, objs, mt, order, census = (_host(env, k)[e] for k in ('pool_mat', 'pool_objs', 'pool_mt', 'pool_chunk_order', 'pool_census'))
  return [dict(mat=mat[i], objs=objs[i][:hdr[i]['nobj']], mt=mt[i], mt_pos=int(hdr[i]['mt_pos']), chunk_order=order[i][:hdr[i]['nchunks_seen']],
               census=census[i]) for i in range(env.num_envs)]


def assert_same_worlds(a, b, what):
  for i, (x, y) in enumerate(zip(a, b)):
    assert len(x['objs']) > 2 and x['mt_pos'] != abi.MT_N, 'an empty world proves nothing'
    for k in FIELDS:
      assert np.array_equal(x[k], y[k]), f'{what}, env {i}: {k}'


@pytest.mark.parametrize('shape', list(SHAPES))
def test_three_forms_make_the_same_world_on_the_device(shape):
  from crafter_amd import BatchedEnv
  n, area, view, size = SHAPES[shape]
  seeds = [8100 + 7 * i for i in range(n)]
  kw = dict(seeds=seeds, area=area, view=view, size=size, device='cuda:0')
  a = BatchedEnv(n, gen_period=-1, **kw)
  a.reset()
  a.reset()
  fused_row_2 = row_worlds(a)
  a.reset()
  fused_row_3 = row_worlds(a)
  a.check_errors()

  b = BatchedEnv(n, gen_period=1, **kw)
  b.reset()
  torch.cuda.synchronize()
  assert_same_worlds(fused_row_2, entry_worlds(b, 2), 'episode 2: crafter_reset_kernel row / gen_body entry')
  b.step(torch.zeros(n, dtype=torch.int32, device='cuda:0'))
  torch.cuda.synchronize()
  assert_same_worlds(fused_row_3, entry_worlds(b, 3), 'episode 3: crafter_reset_kernel row / generation kernels entry')
  b.check_errors()
  assert b.pool_status()['state'] == 'running'
