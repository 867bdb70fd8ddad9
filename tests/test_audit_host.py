"""The audit of env rows, the parts that need no GPU: crafter_audit's body on the CPU (tests/hostsim/audit_host.cpp) stays silent
on every path that writes rows -- step, rollout, subset step, subset rollout, auto-resets from the pool and inline, authored
worlds, edit tapes, the rule-branch atlas, copied / saved / loaded rows -- and names each corruption of tests/audit_cases.py by
bit and detail; the numpy mirror (crafter_amd.audit_host) agrees with it integer for integer; the sanitised stand-alone program
reads clean, corrupted and random rows without a finding; masks, constants, the entry point, the kernel's budget."""
import pathlib
import re
import shutil
import subprocess

import numpy as np
import pytest

import crafter_amd
from crafter_amd import abi, edits as E, state
from tests import audit_cases as cases

ROOT = pathlib.Path(__file__).resolve().parent.parent
GEOS = {
    '64x64': dict(area=(64, 64)),
    '42x30': dict(area=(42, 30), view=(7, 9), size=(84, 72)),   # W H = 1260: the byte path
    '48x40': dict(area=(48, 40)),
    '256x256': dict(area=(256, 256)),                            # objmap is state, FarSlot, a workgroup per env
}
LENGTH = 200   # an episode ends in its first night (daylight < 0.5 from step 148 on): balance passes by night, then an auto-reset


def _hostsim(seeds, **kw):
  from tests.hostsim.driver import HostSimEnv
  return HostSimEnv(seeds, render_obs=False, **kw)


def _ctx(hs):
  from tests.hostsim import audit_build as ab
  return cases.Ctx(hs.cfg, hs.tab.rules, ab.map_is_state(hs))


def _assert_clean(hs, where, mirror=False):
  from tests.hostsim import audit_build as ab
  flags, detail = ab.audit(hs)
  bad = np.nonzero(flags)[0]
  assert not len(bad), f'{where}: env {bad[0]} fails {[n for b, n in enumerate(abi.AUDIT_NAMES) if flags[bad[0]] >> b & 1]}, detail {detail[bad[0]].tolist()}'
  assert (detail == -1).all(), where
  if mirror:
    mf, md = state.audit_host(hs.buf, hs.cfg, hs.tab.rules, not ab.map_is_state(hs))
    assert np.array_equal(mf, flags) and np.array_equal(md, detail), where


# ------------------------------------------------------------------ a. clean runs
@pytest.mark.parametrize('pool', [True, False], ids=['pool', 'inline'])
@pytest.mark.parametrize('geo', list(GEOS))
def test_clean_on_every_step_path(geo, pool):
  """Five envs through two nights and two auto-resets each, the calls dealt in turn to step, rollout, subset step and subset
  rollout: no row fails anything after any call, before the first reset every row says NOT_RESET and nothing else."""
  from tests.hostsim import audit_build as ab, rollout_envs_build as rb, subset_build as sb
  n = 5
  hs = _hostsim([70 + i for i in range(n)], length=LENGTH, auto_reset=True, pool=pool, **GEOS[geo])
  assert ab.map_is_state(hs) == (geo == '256x256') and bool(ab.lib().hostsim_audit_in_wave(ab.C.byref(hs.cfg))) == (geo != '256x256')
  assert ab.lib().hostsim_audit_lds_bytes(ab.C.byref(hs.cfg)) == {'64x64': 1440, '42x30': 512, '48x40': 688, '256x256': 19872}[geo]   # 
  flags, detail = ab.audit(hs)
  assert (flags == abi.AUDIT_NOT_RESET).all() and (detail == [0, -1, -1, -1]).all()
  hs.reset()
  _assert_clean(hs, 'reset', mirror=True)
  rs = np.random.RandomState(3)
  marks, rmarks = sb.Marks(n), rb.Marks(n)
  daylight = np.asarray(hs.tab.daylight)
  night = balance = t = call = 0
  while t < 2 * LENGTH + 30:
    kind = call % 4
    call += 1
    before = hs.rec['step'].copy()
    if kind == 0:
      hs.step(rs.randint(0, 17, n).astype(np.int32))
      steps = 1
    elif kind == 1:
      steps = 3
      hs.step_n(rs.randint(0, 17, (steps, n)).astype(np.int32))
    else:
      idx = rs.permutation(n)
      k = int(rs.randint(1, n))
      steps = 1 if kind == 2 else 2
      for half in (idx[:k], idx[k:]):   # (two calls that together name every env: the batch stays in step)
        if kind == 2:
          assert sb.step_envs(hs, marks, half, rs.randint(0, 17, len(half))) == 0
        else:
          assert rb.rollout_envs(hs, rmarks, half, rs.randint(0, 17, (steps, len(half))))[0] == 0
        _assert_clean(hs, f'{geo} call {call} (half)')
    t += steps
    _assert_clean(hs, f'{geo} call {call} kind {kind} at step {t}', mirror=call % 16 == 0)
    for a, z in zip(before, hs.rec['step']):   # the steps an env played in this call (none counted across a reset)
      played = np.arange(a + 1, z + 1)
      night += int((daylight[played] < 0.5).sum())
      balance += int(((daylight[played] < 0.5) & (played % 10 == 0)).sum())   # (env.py:160: the balance pass of every tenth step)
  assert night >= 100 and balance >= 8, (night, balance)
  assert int((hs.rec['episode'] - 1).sum()) >= 4 and not hs.rec['status'].any()
  if pool:
    assert hs.buf['pool_stats'][0] > 0
  _assert_clean(hs, 'end', mirror=True)


def test_clean_behind_authored_worlds_edits_and_copies():
  """tests/edits_cases.py's three cases: reset into authored worlds, every edit op applied from tapes between the steps of a run
  into the night; then rows copied, saved and loaded the way copy_envs / save_state / load_state move them (every buffer of
  state.STORE_BUFFERS; the harness has no copy body, the GPU test runs the kernels).  Silent throughout."""
  from tests import edits_cases as ec
  from tests.hostsim import edits_build as eb, worlds_build
  from tests.hostsim.driver import HostSimEnv
  kinds = {int(op[0]) for sched in ec.SCHEDULES for ops in sched.values() for op in E.encode(ec.GEO, ops, 1)[0]}
  assert kinds == set(range(abi.EDIT_KINDS)), kinds
  hs = HostSimEnv(list(ec.SEEDS), auto_reset=False, render_obs=False)
  assert worlds_build.reset_worlds(hs, ec.bank_of(hs, range(3))) == 0
  _assert_clean(hs, 'authored worlds', mirror=True)
  for t in range(ec.T):
    named = [i for i in range(3) if t in ec.SCHEDULES[i]]
    if named:
      assert eb.edit(hs, named, [ec.SCHEDULES[i][t] for i in named]) == 0
      _assert_clean(hs, f'edit before step {t + 1}', mirror=True)
    hs.step(np.array([ec.tape(i)[t] for i in range(3)], np.int32))
    _assert_clean(hs, f'step {t + 1}')
  assert (np.asarray(hs.tab.daylight)[hs.rec['step']] < 0.5).all() and not hs.rec['status'].any()
  saved = {k: hs.buf[k].copy() for k in state.STORE_BUFFERS}
  for k in state.STORE_BUFFERS:
    hs.buf[k][2] = hs.buf[k][0]   # copy_envs([0], [2])
  _assert_clean(hs, 'copy', mirror=True)
  hs.step(np.array([5, 1, 5], np.int32))
  _assert_clean(hs, 'step behind the copy')
  for k in state.STORE_BUFFERS:
    hs.buf[k][[0, 1]] = saved[k][[2, 1]]   # load_state(store, idx=[0, 1], rows=[2, 1])
  _assert_clean(hs, 'load', mirror=True)
  hs.step(np.array([2, 3, 4], np.int32))
  _assert_clean(hs, 'step behind the load', mirror=True)


@pytest.mark.parametrize('geometry', ['default', '48x40', '256'])
def test_clean_on_the_rule_branch_atlas(geometry):
  """The authored worlds of tests/atlas_cases.py pin every objects.py branch; each step of their tapes leaves rows that are rows."""
  from tests import atlas_cases as ac
  from tests.hostsim import worlds_build
  from tests.hostsim.driver import HostSimEnv
  g = ac.GEOMETRIES[geometry]
  hs = HostSimEnv(ac.SEEDS, auto_reset=False, render_obs=False, **g)
  assert worlds_build.reset_worlds(hs, ac.bank_of(hs, g['area'])) == 0
  _assert_clean(hs, 'atlas reset', mirror=True)
  tapes = ac.tapes()
  for t in range(1, ac.T + 1):
    hs.step(tapes[t - 1])
    _assert_clean(hs, f'atlas step {t}', mirror=t % 8 == 0)
  assert not hs.rec['status'].any()


# ------------------------------------------------------------------ b. corruptions
@pytest.fixture(scope='module', params=['64x64', '256x256'])
def batch(request):
  """Six envs 12 steps into their episodes (the zombies of the generator still stand: daylight despawns them), clean; never
  modified (the cases work on copies)."""
  from tests.hostsim import audit_build as ab
  hs = _hostsim([900 + i for i in range(6)], length=10000, auto_reset=True, **GEOS[request.param])
  hs.reset()
  rs = np.random.RandomState(9)
  for _ in range(12):
    hs.step(rs.randint(0, 17, 6).astype(np.int32))
  _assert_clean(hs, 'the batch', mirror=True)
  ctx = _ctx(hs)
  return hs, ctx, {k: v for k, v in ab.copy_buffers(hs).items() if k != 'objmap' or ctx.map_state}


def test_finds_each_corruption(batch, tmp_path):
  """Every case of the table on rows 1 and 3 of a copy of the batch: exactly the case's bits and its detail on those rows, 0 and
  -1 on the others; the numpy mirror says the same integers; and the sanitised stand-alone program, every buffer of exactly its
  size, reads the corrupted batch without a finding and prints them too."""
  from tests.hostsim import audit_build as ab
  hs, ctx, clean = batch
  names = list(cases.cases(ctx))
  assert len(names) == (25 if ctx.map_state else 22)
  for name in names:
    buf, want = cases.corrupted(clean, name, (1, 3), ctx)
    flags, detail = ab.audit(hs, buf=buf)
    cases.check(flags, detail, want, name)
    mf, md = state.audit_host(buf, hs.cfg, hs.tab.rules, not ctx.map_state)
    assert np.array_equal(mf, flags) and np.array_equal(md, detail), (name, mf, flags, md[[1, 3]], detail[[1, 3]])
    ab.dump(hs, tmp_path / 'case.blob', buf=buf)
    rows = ab.run_sanitized(tmp_path / 'case.blob')
    assert rows == [(int(f), [int(v) for v in d]) for f, d in zip(flags, detail)], name
  for k in clean:   # the fixture's buffers are as they were
    assert np.array_equal(clean[k], hs.buf[k])


@pytest.mark.parametrize('geo', list(GEOS))
def test_sanitized_program_on_clean_and_random_rows(geo, tmp_path):
  """The stand-alone program over three clean rows under a mask, and over rows of uniformly random bytes -- one of them with
  episode forced to non-zero counts, so that every phase runs on garbage: exits clean (the proof that the body bounds what it
  reads), prints what the body loaded into Python computes, and the mirror agrees on garbage as well."""
  from tests.hostsim import audit_build as ab
  hs = _hostsim([41, 42, 43], length=15, auto_reset=True, **GEOS[geo])
  hs.reset()
  rs = np.random.RandomState(5)
  for t in range(40):
    hs.step(rs.randint(0, 17, size=3).astype(np.int32))
  mask = np.array([1, 0, 1], np.uint8)
  ab.dump(hs, tmp_path / 'clean.blob', mask=mask)
  assert ab.run_sanitized(tmp_path / 'clean.blob') == [(0, [-1] * 4), None, (0, [-1] * 4)]
  buf = ab.copy_buffers(hs)
  for k in buf:
    raw = buf[k].view(np.uint8)
    raw[...] = rs.randint(0, 256, size=raw.shape, dtype=np.uint8)
  rec = state.rec_view(buf['rec'])
  rec['episode'] = [0, 7, -3]
  rec['nobj'][2], rec['nchunks_seen'][2] = hs.cfg.max_objects - 1, 5   # (counts in range: the passes run their full length)
  flags, detail = ab.audit(hs, buf=buf)
  assert flags[0] == abi.AUDIT_NOT_RESET and (flags[1:] & abi.AUDIT_NOT_RESET == 0).all() and (flags[1:] != 0).all()
  assert flags[1] & abi.AUDIT_REC and flags[2] & abi.AUDIT_MATERIAL and flags[2] & abi.AUDIT_OBJECT
  ab.dump(hs, tmp_path / 'random.blob', buf=buf)
  assert ab.run_sanitized(tmp_path / 'random.blob') == [(int(f), [int(v) for v in d]) for f, d in zip(flags, detail)]
  mf, md = state.audit_host(buf, hs.cfg, hs.tab.rules, not ab.map_is_state(hs))
  assert np.array_equal(mf, flags) and np.array_equal(md, detail), (mf, flags, md, detail)


# ------------------------------------------------------------------ c. mask, tail, arguments
def test_masked_rows_keep_a_sentinel():
  """Five envs under a row mask, written into sentinel-filled outputs inside larger buffers: masked rows and the words around
  the outputs stay as they were (the body is also called for one env beyond the batch); null outputs are refused."""
  from tests.hostsim import audit_build as ab
  hs = _hostsim([11, 12, 13, 14, 15], **GEOS['64x64'])
  hs.reset()
  hs.buf['census'][3][2] += 1   # (a finding in a row the mask names)
  hs.buf['census'][1][2] += 1   # ... and one in a row it leaves out
  sentinel = np.int32(0x5E5E5E5E)
  raw_flags, raw_detail = np.full(5 + 4, sentinel), np.full(5 * 4 + 4, sentinel)
  flags, detail = raw_flags[2:7], raw_detail[2:22].reshape(5, 4)
  mask = np.array([1, 0, 0, 1, 1], np.uint8)
  ab.audit(hs, mask=mask, flags=flags, detail=detail)
  assert flags.tolist() == [0, sentinel, sentinel, abi.AUDIT_CREATURES, 0]
  assert (detail[[1, 2]] == sentinel).all() and (detail[[0, 4]] == -1).all() and detail[3].tolist()[:2] == [8, 2]
  assert (raw_flags[:2] == sentinel).all() and (raw_flags[7:] == sentinel).all() and (raw_detail[:2] == sentinel).all() and (raw_detail[22:] == sentinel).all()
  mf, md = state.audit_host(hs.buf, hs.cfg, hs.tab.rules, True, mask=mask)
  assert mf.tolist() == [0, 0, 0, abi.AUDIT_CREATURES, 0] and np.array_equal(md[3], detail[3])
  args = (ab.C.byref(hs.cfg), ab.C.byref(hs.tb), ab.C.byref(hs.st), 0, None)
  assert ab.lib().hostsim_audit(*args, None, ab._p(detail)) == 1 and ab.lib().hostsim_audit(*args, ab._p(flags), None) == 1


# ------------------------------------------------------------------ d. the library
def test_constants_match_the_c_header(tmp_path):
  """abi.AUDIT_* against CRAFTER_AUDIT_* as a C compiler reads include/crafter_hip_audit.h, pedantic C99 by itself."""
  if not shutil.which('gcc'):
    pytest.skip('needs gcc')
  names = list(abi.AUDIT_NAMES)
  header = (ROOT / 'include' / 'crafter_hip_audit.h').read_text()
  assert set(re.findall(r'\bCRAFTER_AUDIT_([A-Z_]+)\b', header)) == set(names) | {'BITS'}
  src = tmp_path / 'audit.c'
  src.write_text('#include <stdio.h>\n#include "crafter_hip_audit.h"\nint main(void) {\n' +
                 ''.join(f'  printf("{n} %ld\\n", (long)CRAFTER_AUDIT_{n});\n' for n in names + ['BITS']) + '  return 0;\n}\n')
  subprocess.run(['gcc', '-std=c99', '-pedantic', '-Wall', '-Werror', f'-I{ROOT / "include"}', str(src), '-o', str(tmp_path / 'audit')], check=True)
  out = subprocess.run([str(tmp_path / 'audit')], capture_output=True, text=True, check=True).stdout
  got = {k: int(v) for k, v in (line.split() for line in out.splitlines())}
  assert got == dict({n: getattr(abi, f'AUDIT_{n}') for n in names}, BITS=abi.AUDIT_BITS)
  assert [getattr(abi, f'AUDIT_{n}') for n in names] == [1 << b for b in range(abi.AUDIT_BITS)] and crafter_amd.AUDIT_NAMES is abi.AUDIT_NAMES


def test_entry_point_declared_listed_and_exported():
  """crafter_audit extends the boundary from a header of its own, lib.EXTENSIONS lists it, build.sources() holds the header and
  the library exports it; the core header and lib.SIGNATURES stay the pinned pair."""
  from crafter_amd import build, lib as hiplib
  header = (ROOT / 'include' / 'crafter_hip_audit.h').read_text()
  assert 'crafter_audit' not in (ROOT / 'include' / 'crafter_hip.h').read_text() and 'crafter_audit' not in hiplib.SIGNATURES
  assert ROOT / 'include' / 'crafter_hip_audit.h' in build.sources() and ROOT / 'crafter_amd' / 'csrc' / 'audit.hpp' in build.sources()
  assert re.search(r'\bint crafter_audit\(crafter_handle\* h, const uint8_t\* mask, int32_t\* flags, int32_t\* detail, void\* stream\);', header)
  nm = subprocess.run(['nm', '-D', '--defined-only', str(build.build())], capture_output=True, text=True, check=True).stdout
  assert 'crafter_audit' in set(re.findall(r'\b(crafter_[a-z_]+)$', nm, re.M))
  where, restype, argtypes = hiplib.EXTENSIONS['crafter_audit']
  assert where == 'crafter_hip_audit.h' and restype is hiplib.i32 and list(argtypes) == [hiplib.vp] * 5
  so = hiplib.load()
  assert so.crafter_audit.restype is hiplib.i32 and so.crafter_abi_version() == 7


def test_audit_kernel_budget():
  """Four instances (one wave or 256 threads, objmap state or not): no scratch, no spill, and registers for eight waves per SIMD."""
  from crafter_amd import build
  usage = {k: v for k, v in build.resource_usage().items() if k.startswith('crafter_audit_kernel')}
  assert sorted(usage) == ['crafter_audit_kernel<256,0>', 'crafter_audit_kernel<256,1>', 'crafter_audit_kernel<64,0>', 'crafter_audit_kernel<64,1>']
  for name, u in usage.items():
    assert u['scratch'] == 0 and u.get('vgpr_spill', 0) == 0 and u.get('sgpr_spill', 0) == 0, (name, u)
    assert u['vgprs'] <= 64 and u['occupancy'] >= 8, (name, u)
