"""crafter_step_final without a GPU: final_reset_body (csrc/reset_bodies.hpp) through the CPU harness (tests/hostsim/final_host.cpp)
behind the step bodies run with gen_parity = -1, against the oracle -- terminal frame, terminated, the terminal state's symbolic
pair, and obs / reward / done of every step --, against the plain step path on a second harness env, and once as a stand-alone
program built with -fsanitize=address,undefined.  The entry point's declaration and export are checked on the library."""
import pathlib
import re
import subprocess

import numpy as np
import pytest

from tests import final_ref as fr
from tests.parity import sha8

ROOT = pathlib.Path(__file__).resolve().parent.parent


def _hostsim(seeds, **kw):
  from tests.hostsim.driver import HostSimEnv
  hs = HostSimEnv(list(seeds), auto_reset=True, **{**dict(length=fr.LENGTH), **kw})
  hs.reset()
  return hs


def _compare_with_oracle(seeds, steps=fr.STEPS, split=False, cases=False, **kw):
  """Plays the tapes with hostsim_step_final and checks every step against the oracle; -> finished (env, t) pairs."""
  from tests.hostsim import final_build as fb
  runs, fin = fr.reference(tuple(seeds), steps)
  if cases:
    fr.assert_cases(seeds, fin)
  hs = _hostsim(seeds, **kw)
  out = fb.FinalBuffers(hs)
  acts = np.stack([fr.tape(s, steps) for s in seeds], axis=1)
  nth = [0] * len(seeds)
  seen = []
  for t in range(steps):
    keep = (out.obs.copy(), out.terminated.copy(), out.local.copy(), out.stats.copy())
    queued = fb.step_final(hs, acts[t], out, split=split)
    assert queued == int(hs.done.astype(bool).sum())
    for i, (s, run) in enumerate(zip(seeds, runs)):
      assert bool(hs.done[i]) == run['done'][t] and np.float32(hs.reward[i]) == run['reward'][t], (s, t)
      if hs.cfg.render_obs:
        assert sha8(hs.obs[i]) == run['obs_sha'][t], f'obs of seed {s} step {t}'
      if hs.done[i]:
        f = fin[i][nth[i]]
        nth[i] += 1
        assert f['t'] == t
        if hs.cfg.render_obs:
          assert sha8(out.obs[i]) == f['sha'], f'final_obs of seed {s} step {t} (daylight {f["daylight"]:.2f}, asleep {f["sleeping"]})'
        else:
          assert (out.obs[i] == fb.FinalBuffers.PATTERN).all()
        assert out.terminated[i] == int(f['terminated']), (s, t)
        assert np.array_equal(out.local[i], f['local']), (s, t)
        assert np.array_equal(out.stats[i].view(np.uint32), f['stats'].view(np.uint32)), (s, t, out.stats[i], f['stats'])
        seen.append((i, t))
      else:   # untouched rows
        assert np.array_equal(out.obs[i], keep[0][i]) and out.terminated[i] == keep[1][i]
        assert np.array_equal(out.local[i], keep[2][i]) and np.array_equal(out.stats[i], keep[3][i])
  assert nth == [len(f) for f in fin]
  return hs, seen


@pytest.mark.parametrize('pool', [False, True], ids=['inline', 'pool'])
def test_final_body_equals_oracle(pool):
  hs, seen = _compare_with_oracle(fr.HOST_SEEDS, cases=True, pool=pool)
  assert len(seen) >= len(fr.HOST_SEEDS)
  stats = hs.buf['pool_stats']
  if pool:   # every world after the first came from the pool (generation runs right after each call here)
    assert stats[0] == len(seen) and stats[1] == 0
  else:
    assert stats[0] == 0


def test_final_body_behind_the_split_step_and_without_frames():
  _compare_with_oracle(fr.HOST_SEEDS[:3], steps=120, split=True, pool=True)   # 111 (t=52), 117 (t=107): day; 101 plays on
  _compare_with_oracle(fr.HOST_SEEDS[2:4], steps=fr.STEPS, render_obs=False)


def test_final_body_large_world():
  """area (144, 144): the maps and the slot table stay in global memory (big_layout step, big_reset_layout adoption in place)."""
  seeds, steps, kw = (100, 101), 45, dict(area=(144, 144), length=20)
  from tests.hostsim import final_build as fb
  runs, fin = fr.reference(seeds, steps, tuple(sorted(kw.items())))
  assert all(len(f) == 2 for f in fin)
  for pool in (False, True):
    hs = _hostsim(seeds, pool=pool, **kw)
    assert not hs.lib.hostsim_slot_map_derived(__import__('ctypes').byref(hs.cfg))
    out = fb.FinalBuffers(hs)
    nth = [0, 0]
    for t in range(steps):
      fb.step_final(hs, [fr.tape(s, steps)[t] for s in seeds], out)
      for i, run in enumerate(runs):
        assert bool(hs.done[i]) == run['done'][t] and sha8(hs.obs[i]) == run['obs_sha'][t], (pool, i, t)
        if hs.done[i]:
          f = fin[i][nth[i]]
          nth[i] += 1
          assert sha8(out.obs[i]) == f['sha'] and out.terminated[i] == int(f['terminated']), (pool, i, t)
          assert np.array_equal(out.local[i], f['local']) and np.array_equal(out.stats[i].view(np.uint32), f['stats'].view(np.uint32))
    assert nth == [2, 2]
    assert hs.buf['pool_stats'][0] == (4 if pool else 0)


def test_final_path_leaves_the_state_of_the_plain_path():
  """Same seeds through hs.step() and through step_final: obs, reward, done, terminal rows, every state buffer; then swapped."""
  from tests.hostsim import final_build as fb
  seeds = fr.HOST_SEEDS[:2]
  for pool in (False, True):
    a, b = _hostsim(seeds, pool=pool), _hostsim(seeds, pool=pool)
    out_a, out_b = fb.FinalBuffers(a), fb.FinalBuffers(b)
    acts = np.stack([fr.tape(s, 140) for s in seeds], axis=1)
    for t in range(140):
      if t < 110:
        a.step(acts[t]), fb.step_final(b, acts[t], out_b)
      else:
        fb.step_final(a, acts[t], out_a), b.step(acts[t])
      assert np.array_equal(a.obs, b.obs) and np.array_equal(a.reward, b.reward) and np.array_equal(a.done, b.done), t
      for name in ('mat', 'mt', 'rec', 'chunk_order', 'chunk_seen', 'census', 'terminal', 'pool_stats', 'gen_latest', 'pool_hdr'):
        assert np.array_equal(a.buf[name], b.buf[name]), (pool, t, name)
      for i in range(len(seeds)):
        sa, sb = a.snapshot(i), b.snapshot(i)
        assert sa['objects'] == sb['objects'] and np.array_equal(sa['occupied'], sb['occupied']), (pool, t, i)
    assert a.rec['episode'].min() >= 1


def test_refused_without_auto_reset():
  from tests.hostsim import final_build as fb
  from tests.hostsim.driver import HostSimEnv
  hs = HostSimEnv([3], length=5)
  hs.reset()
  assert fb.step_final(hs, [0], fb.FinalBuffers(hs)) == -1


def test_sanitized_standalone_program(tmp_path):
  """final_main.cpp built with -fsanitize=address,undefined plays seed 108 (dies asleep, at night) from a dumped harness env; its
  lines equal the shared library's run."""
  from tests.hostsim import final_build as fb
  seed, steps = 108, fr.STEPS
  runs, fin = fr.reference(fr.HOST_SEEDS, steps)
  t_end = fin[fr.HOST_SEEDS.index(seed)][0]['t'] + 3
  acts = fr.tape(seed, steps)[:t_end].reshape(-1, 1)
  hs = _hostsim([seed], pool=True)
  blob = tmp_path / 'final.blob'
  fb.dump(hs, acts, blob)
  out = fb.FinalBuffers(hs)
  want = []
  for t in range(t_end):
    fb.step_final(hs, acts[t], out)
    if hs.done[0]:
      want.append(f'{t} 0 {int(out.terminated[0])} {fb.fnv(out.obs[0]):016x} {fb.fnv(out.local[0]):016x} {fb.fnv(out.stats[0]):016x} {fb.fnv(hs.obs[0]):016x}')
  assert len(want) == 1
  proc = subprocess.run([str(fb.build_sanitized()), str(blob)], capture_output=True, text=True, timeout=600)
  assert proc.returncode == 0, proc.stderr[-2000:]
  assert proc.stdout.split('\n')[:-1] == want


# ------------------------------------------------------------------ the library
def test_entry_point_declared_listed_and_exported():
  from crafter_amd import build, lib as hiplib
  header = (ROOT / 'include' / 'crafter_hip.h').read_text()
  path = build.build()
  nm = subprocess.run(['nm', '-D', '--defined-only', str(path)], capture_output=True, text=True, check=True).stdout
  exported = set(re.findall(r'\b(crafter_[a-z_]+)$', nm, re.M))
  assert re.search(r'\bint crafter_step_final\(crafter_handle\* h, const int32_t\* actions, uint8_t\* obs, float\* reward, uint8_t\* done,\s*'
                   r'uint8_t\* final_obs, uint8_t\* terminated, uint8_t\* final_local, float\* final_stats, void\* stream\);', header)
  assert 'crafter_step_final' in hiplib.EXPORTS and 'crafter_step_final' in exported
  so = hiplib.load()
  assert len(so.crafter_step_final.argtypes) == 10
  assert so.crafter_abi_version() == 7

