"""Level sets without a GPU: crafter_set_levels / crafter_level_ids declared, listed and exported; `pick` (csrc/env_levels.hpp) on
hand-made inputs against crafter_amd.levels_pick; the set-levels and level-ids bodies on hand-made arrays; an env under a table
behind the CPU harness against the oracle, pool on and off; BatchedEnv's host-side argument checks; the kernels' resource usage."""
import ctypes as C
import pathlib
import re
import subprocess

import numpy as np
import pytest

import crafter_amd
from crafter_amd import abi, state, tables
from tests.parity import assert_same

ROOT = pathlib.Path(__file__).resolve().parent.parent
M64 = 0xFFFFFFFFFFFFFFFF


# ------------------------------------------------------------------ the library
def test_entry_points_declared_listed_and_exported():
  from crafter_amd import build, lib as hiplib
  header = (ROOT / 'include' / 'crafter_hip.h').read_text()
  path = build.build()
  nm = subprocess.run(['nm', '-D', '--defined-only', str(path)], capture_output=True, text=True, check=True).stdout
  exported = set(re.findall(r'\b(crafter_[a-z_]+)$', nm, re.M))
  assert re.search(r'\bint crafter_set_levels\(crafter_handle\* h, const uint64_t\* seed_lane, const int32_t\* episode,\s*'
                   r'const uint32_t\* cum, int32_t n_levels, uint64_t key, void\* stream\);', header)
  assert re.search(r'\bint crafter_level_ids\(crafter_handle\* h, const uint8_t\* mask, int32_t\* ids, void\* stream\);', header)
  section = header[header.index('Level sets'):]
  assert 'additive under abi revision 7: a binding looks them up by name' in section.lower()
  assert 'if that episode began while this table was set' in section.lower()
  for name in ('crafter_set_levels', 'crafter_level_ids'):
    assert name in hiplib.EXPORTS and name in exported
  so = hiplib.load()
  assert len(so.crafter_set_levels.argtypes) == 7 and len(so.crafter_level_ids.argtypes) == 4
  assert so.crafter_abi_version() == 7


def test_level_kernels_budget():
  """One thread per entry / env: no scratch, no spilled register; the seeding kernel of the pool keeps its eight waves per SIMD
  with the hash and the search in front of it."""
  from crafter_amd import build
  usage = build.resource_usage()
  for name in ('crafter_set_levels_kernel', 'crafter_level_ids_kernel'):
    u = usage[name]
    assert u['scratch'] == 0 and u.get('vgpr_spill', 0) == 0, (name, u)
  u = usage['crafter_gen_seed_kernel<1>']
  assert u['occupancy'] == 8 and u['scratch'] == 0 and u.get('vgpr_spill', 0) == 0, u


def test_env_levels_header_states_what_it_supersedes():
  head = (ROOT / 'crafter_amd' / 'csrc' / 'env_levels.hpp').read_text().splitlines()[:6]
  assert 'supersede' in ' '.join(head) and 'DESIGN.md 9.0' in ' '.join(head)


# ------------------------------------------------------------------ pick on hand-made inputs
LANES = np.array([0, 1, M64, 2 ** 63, 0x0123456789ABCDEF, 12345, M64 - 1, 2 ** 32], np.uint64)
KS = [1, 2, 2 ** 31 - 3]


def _pairs():
  lanes = np.repeat(LANES, len(KS))
  ks = np.tile(np.array(KS, np.int32), len(LANES))
  # ... and a few thousand more lanes, so that every entry of a small table and many of a large one are hit
  rs = np.random.RandomState(5)
  more = rs.randint(0, 2 ** 63, size=4000, dtype=np.int64).astype(np.uint64) * np.uint64(2) + rs.randint(0, 2, size=4000).astype(np.uint64)
  return np.concatenate([lanes, more]), np.concatenate([ks, rs.choice(KS, size=4000).astype(np.int32)])


def _table(K, cum=None, key=0):
  from tests.hostsim import levelset_build as lb
  cfg, _ = tables.make_config(4, tables.load_rules())
  rec = np.zeros((4, abi.REC_DTYPE.itemsize), np.uint8)
  st = abi.StatePtrs(rec=rec.ctypes.data_as(C.c_void_p).value)
  t = lb.Table()
  lanes = np.arange(K, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(7)
  eps = (np.arange(K, dtype=np.int32) % 5) + 1
  t.set(cfg, st, lanes, eps, cum, key)
  t.keep = (cfg, rec, st, lanes, eps)
  return t


@pytest.mark.parametrize('key', [0, 0xDEADBEEFCAFEF00D], ids=['key0', 'key64'])
@pytest.mark.parametrize('K', [1, 2, 3, 65536])
def test_pick_uniform_equals_the_mirror(K, key):
  lanes, ks = _pairs()
  got = _table(K, None, key).pick(lanes, ks)
  want = crafter_amd.levels_pick(lanes, ks, K, None, key)
  assert want.dtype == np.int32 and np.array_equal(got, want)
  assert got.min() >= 0 and got.max() < K
  if K in (2, 3):
    assert set(got.tolist()) == set(range(K))
  if K == 65536:
    assert len(set(got.tolist())) > 3000


WEIGHTED = {
    'leading-zero': [0, 1, 3],
    'inner-zero': [2, 0, 0, 5, 1],
    'trailing-zero': [1, 2, 0],
    'all-but-one-zero': [0, 1, 0],
    'single': [7],
    'floats': [0.5, 0.125, 0.0, 0.375],
}


@pytest.mark.parametrize('name', sorted(WEIGHTED))
def test_pick_weighted_equals_the_mirror(name):
  w = WEIGHTED[name]
  K = len(w)
  cum = state.levels_cum(w)
  total = sum(w)
  acc = np.cumsum(np.asarray(w, np.float64))
  assert cum.dtype == np.uint32 and cum.tolist() == [min(int(2 ** 32 * a / total), 2 ** 32 - 1) for a in acc]   # (exact in doubles for these)
  lanes, ks = _pairs()
  got = _table(K, cum, 3).pick(lanes, ks)
  want = crafter_amd.levels_pick(lanes, ks, K, cum, 3)
  assert np.array_equal(got, want)
  drawn = set(got.tolist())
  assert drawn == {j for j in range(K) if w[j] > 0}   # a level of weight 0 is not drawn, every other one is


def test_pick_weighted_last_entry_counts_as_full():
  """cum[K - 1] < 2^32 - 1: whatever lies above it still goes to the last entry.  And a large weighted table (the search's 16
  rounds)."""
  lanes, ks = _pairs()
  cum = np.array([2 ** 30, 2 ** 31, 2 ** 31 + 5], np.uint32)
  got = _table(3, cum).pick(lanes, ks)
  assert np.array_equal(got, crafter_amd.levels_pick(lanes, ks, 3, cum)) and set(got.tolist()) == {0, 1, 2}
  assert abs((got == 2).mean() - 0.5) < 0.05
  rs = np.random.RandomState(9)
  w = rs.randint(0, 4, size=65536)
  cum = state.levels_cum(w)
  got = _table(65536, cum, 1).pick(lanes, ks)
  assert np.array_equal(got, crafter_amd.levels_pick(lanes, ks, 65536, cum, 1))
  assert (w[got] > 0).all()


def test_level_seed_is_the_entrys_world_seed():
  from tests.hostsim import driver, levelset_build as lb
  t = _table(3, None, 5)
  cfg, rec, st, lanes, eps = t.keep
  for lane, k in ((0, 1), (M64, 2), (99, 2 ** 31 - 3)):
    j = int(crafter_amd.levels_pick([lane], [k], 3, None, 5)[0])
    assert lb.lib().hostsim_level_seed(t.ptr, lane, k) == driver.lib().hostsim_world_seed(int(lanes[j]), int(eps[j]))
    assert lb.lib().hostsim_level_seed(None, lane, k) == driver.lib().hostsim_world_seed(lane, k)
  t.set(cfg, st, None, None)   # cleared: (lane, k) itself
  assert lb.lib().hostsim_level_seed(t.ptr, 99, 4) == driver.lib().hostsim_world_seed(99, 4)


# ------------------------------------------------------------------ the bodies on hand-made arrays
N = 300   # two workgroups of the kernel's 256 threads, the second one partly beyond the batch


def _arrays(seed=1):
  rs = np.random.RandomState(seed)
  cfg, _ = tables.make_config(N, tables.load_rules())
  rec = rs.randint(0, 256, size=(N, abi.REC_DTYPE.itemsize)).astype(np.uint8)
  state.rec_view(rec)['episode'] = rs.randint(0, 2 ** 31 - 3, size=N)
  hdr = rs.randint(0, 256, size=(2, N, abi.POOL_HDR_DTYPE.itemsize)).astype(np.uint8)
  latest = rs.randint(5, 1000, size=N).astype(np.int32)
  return cfg, rec, hdr, latest


def _ptrs(rec, hdr=None, latest=None):
  p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p).value
  return abi.StatePtrs(rec=p(rec), pool_hdr=p(hdr), gen_latest=p(latest))


@pytest.mark.parametrize('K', [0, 2, 700], ids=['clear', 'K2', 'K700'])   # fewer levels than envs, more levels than envs
def test_set_levels_body_on_hand_made_arrays(K):
  from tests.hostsim import levelset_build as lb
  cfg, rec, hdr, latest = _arrays()
  rec0, hdr0 = rec.copy(), hdr.copy()
  rs = np.random.RandomState(3)
  lanes = rs.randint(0, 2 ** 63, size=K, dtype=np.int64).astype(np.uint64) * np.uint64(2) + np.uint64(1) if K else None
  eps = rs.randint(1, 9, size=K).astype(np.int32) if K else None
  if K:
    eps[:2] = [0, -4]   # below 1: taken as 1
  cum = state.levels_cum(rs.randint(0, 3, size=K) + (np.arange(K) == 1)) if K == 700 else None
  st = _ptrs(rec, hdr, latest)
  t = lb.Table()
  t.set(cfg, st, lanes, eps, cum, key=0xABCDEF0123456789)
  # no byte of any record changes; every pool header is emptied; gen_latest = rec.episode
  assert np.array_equal(rec, rec0)
  h0, h1 = hdr0.view(abi.POOL_HDR_DTYPE).reshape(2, N), hdr.view(abi.POOL_HDR_DTYPE).reshape(2, N)
  assert (h1['ready'] == 0).all() and (h1['pending'] == 0).all()
  for name in abi.POOL_HDR_DTYPE.names:
    if name not in ('ready', 'pending'):
      assert np.array_equal(h0[name], h1[name]), name
  assert np.array_equal(latest, state.rec_view(rec)['episode'])
  # ids: -1 without a table, else the mirror's -- over (lane, rec.episode) --; masked rows untouched
  r = state.rec_view(rec)
  mask = (rs.randint(0, 3, size=N) > 0).astype(np.uint8) * rs.randint(1, 256, size=N).astype(np.uint8)
  if K == 0:
    assert (t.ids(cfg, st) == -1).all()
    assert (t.ids(cfg, st, table=False) == -1).all()   # a handle that never allocated a table
    want = -1
  else:
    want = crafter_amd.levels_pick(r['seed_lane'], r['episode'], K, cum, 0xABCDEF0123456789)
    assert np.array_equal(t.ids(cfg, st), want)
    assert len(set(want.tolist())) >= 2
    # the table itself: episodes below 1 are stored as 1 (through level_seed: entry j's world seed)
    from tests.hostsim import driver
    for lane, k in zip(r['seed_lane'][:40], r['episode'][:40]):
      j = int(crafter_amd.levels_pick([lane], [k], K, cum, 0xABCDEF0123456789)[0])
      assert lb.lib().hostsim_level_seed(t.ptr, int(lane), int(k)) == driver.lib().hostsim_world_seed(int(lanes[j]), max(int(eps[j]), 1))
  got = t.ids(cfg, st, mask)
  assert (got[mask == 0] == -5).all() and np.array_equal(got[mask != 0], np.broadcast_to(want, (N,))[mask != 0])
  assert np.array_equal(rec, rec0)

  # pool pointers NULL (pool off, failed or absent): only the table is written
  cfg, rec, hdr, latest = _arrays(4)
  before = rec.copy(), hdr.copy(), latest.copy()
  t.set(cfg, _ptrs(rec), lanes, eps, cum)
  assert all(np.array_equal(a, b) for a, b in zip(before, (rec, hdr, latest)))


# ------------------------------------------------------------------ behind the harness, against the oracle
LENGTH = 20
TAB_SEEDS, TAB_EPISODES = [11, 'level-b'], [3, 1]


@pytest.mark.parametrize('pool', [False, True], ids=['inline', 'pool'])
def test_env_under_a_table_plays_the_oracles_levels(pool):
  """Two envs under the table [(11, 3), ('level-b', 1)], over three episode ends each: every episode -- the one reset() starts
  and every automatic one, regenerated inline or adopted from the pool -- is OracleEnv(seed=table seed) at the table's episode,
  the entry being levels_pick(lane, k); rec keeps the env's own lane and counts k; level_ids() is the mirror's."""
  from oracle.crafter_oracle import OracleEnv
  from tests.hostsim import levelset_build as lb
  seeds, key = [3, 4], 21
  lanes = state.seed_lanes(seeds)
  hs = lb.LevelSetEnv(seeds, auto_reset=True, length=LENGTH, pool=pool)
  hs.set_levels(TAB_SEEDS, TAB_EPISODES, key=key)

  def oracle_for(i, k):
    j = int(crafter_amd.levels_pick([lanes[i]], [k], 2, None, key)[0])
    o = OracleEnv(seed=TAB_SEEDS[j], length=LENGTH)
    o._episode = TAB_EPISODES[j] - 1
    return j, o, o.reset()

  def check_start(i, k, where):
    j, o, obs = oracle_for(i, k)
    assert np.array_equal(hs.obs[i], obs), where
    got = dict(hs.snapshot(i))
    assert got['episode'] == k, where
    got['episode'] = TAB_EPISODES[j]
    assert_same(got, o.snapshot(), where)
    assert hs.level_ids()[i] == j, where
    return j, o

  hs.reset()
  cur = [check_start(i, 1, f'reset env {i}') for i in range(2)]
  played = [[cur[i][0]] for i in range(2)]
  k = [1, 1]
  rs = np.random.RandomState(8)
  for t, a in enumerate(rs.randint(0, 17, size=(65, 2))):
    hs.step(a)
    for i in range(2):
      obs, reward, done, _ = cur[i][1].step(int(a[i]))
      assert bool(hs.done[i]) == bool(done) and hs.reward[i] == np.float32(reward), (t, i)
      if done:
        k[i] += 1
        cur[i] = check_start(i, k[i], f'step {t} env {i}')
        played[i].append(cur[i][0])
      else:
        assert np.array_equal(hs.obs[i], obs), (t, i)
  assert min(k) >= 4   # three episode ends each
  for i in range(2):
    got = dict(hs.snapshot(i))
    got['episode'] = TAB_EPISODES[cur[i][0]]
    assert_same(got, cur[i][1].snapshot(), f'final env {i}')
  assert np.array_equal(hs.rec['seed_lane'], lanes) and hs.rec['episode'].tolist() == k
  assert {j for p in played for j in p} == {0, 1}   # both levels were played (the key is chosen so)
  if pool:   # every episode end found its world in the pool
    assert hs.buf['pool_stats'][1] == 0 and hs.buf['pool_stats'][0] == sum(k) - 2

  # clearing the table: the next episodes are the envs' own (lane, k) again
  hs.set_levels(None)
  assert (hs.level_ids() == -1).all()
  if pool:
    assert (hs.pool_hdr['ready'] == 0).all() and np.array_equal(hs.buf['gen_latest'], hs.rec['episode'])
  hs.reset()
  for i in range(2):
    o = OracleEnv(seed=seeds[i], length=LENGTH)
    o._episode = k[i]
    assert np.array_equal(hs.obs[i], o.reset())
    assert_same(hs.snapshot(i), o.snapshot(), f'cleared env {i}')


# ------------------------------------------------------------------ BatchedEnv's host-side checks
def test_host_side_argument_checks():
  from crafter_amd.batched import BatchedEnv
  check = BatchedEnv._check_level_set
  lanes, eps, cum, key = check([0, -3, 'a string', (1, 2)], None, None, 0)
  assert np.array_equal(lanes, state.seed_lanes([0, -3, 'a string', (1, 2)])) and lanes.dtype == np.uint64 and eps is None and cum is None
  assert check([1, 2], 3, None, -1)[1].tolist() == [3, 3] and check([1, 2], 3, None, -1)[3] == M64
  lanes, eps, cum, key = check(np.array([5, 6, 7]), [1, 2, BatchedEnv.MAX_EPISODE], [0, 1, 0], 2 ** 64 + 9)
  assert eps.tolist() == [1, 2, 2 ** 31 - 3] and eps.dtype == np.int32 and key == 9
  assert cum.dtype == np.uint32 and cum.tolist() == [0, 2 ** 32 - 1, 2 ** 32 - 1]
  assert check(list(range(65536)), None, None, 0)[0].size == 65536
  for seeds, episodes, weights in (([], None, None), (list(range(65537)), None, None), ([1, 2, 3], [1, 2], None), ([1, 2, 3], 0, None),
                                   ([1, 2, 3], [1, 1, 0], None), ([1, 2, 3], 2 ** 31 - 2, None), ([1, 2, 3], [1.5, 1, 1], None),
                                   ([1, 2, 3], None, [1, 2]), ([1, 2, 3], None, [1, -1, 1]), ([1, 2, 3], None, [0, 0, 0]),
                                   ([1, 2, 3], None, [1, float('nan'), 1])):
    with pytest.raises(ValueError):
      check(seeds, episodes, weights, 0)
  with pytest.raises(ValueError):
    crafter_amd.levels_pick([1], [1], 0)
  with pytest.raises(ValueError):
    crafter_amd.levels_pick([1], [1], 3, cum=np.zeros(2, np.uint32))


def test_facades_and_cli_offer_set_levels():
  from crafter_amd import BatchedEnv, Env, VecEnvView, run_random
  for cls in (BatchedEnv, Env, VecEnvView):
    assert callable(getattr(cls, 'set_levels'))
  assert callable(BatchedEnv.level_ids)
  assert '--levels' in (ROOT / 'crafter_amd' / 'run_random.py').read_text() and run_random.main is not None
