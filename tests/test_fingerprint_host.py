"""State fingerprints, the parts that need no GPU: crafter_fingerprint's body on the CPU (tests/hostsim/fingerprint_host.cpp)
against the numpy mirror (crafter_amd.fingerprint_host) of HostSimEnv snapshots, the mirror of OracleEnv snapshots against the
body, collisions over a few thousand states, the sanitised stand-alone program, the harness's mask / tail / argument checks, the
new entry point, its constants and the kernel's resource budget."""
import pathlib
import re
import shutil
import subprocess

import numpy as np
import pytest

import crafter_amd
from crafter_amd import abi, state

ROOT = pathlib.Path(__file__).resolve().parent.parent
DEFAULT = dict(area=(64, 64))
# W H = 1260: no multiple of 8 (the padded last unit) nor of 16 (the byte path).  tests/test_configs_hostsim.py plays no such area
# -- its (48, 40) and (40, 48) are multiples of 16 --; this one is tests/test_worlds_host.py's, and (48, 40) rides along
ODD = dict(area=(42, 30), view=(7, 9), size=(84, 72))
SMALL = dict(area=(48, 40))
LARGE = dict(area=(256, 256))   # maps in global memory: the instance that keeps T_NONE holes inside the prefix
U64 = 0xFFFFFFFFFFFFFFFF


def _hostsim(seeds, **kw):
  from tests.hostsim.driver import HostSimEnv
  hs = HostSimEnv(seeds, render_obs=False, **kw)
  hs.reset()
  return hs


def _mirror_rows(hs, parts=abi.FP_ALL):
  rows = [state.fingerprint_host(hs.snapshot(i), hs.rec['seed_lane'][i], parts) for i in range(hs.cfg.num_envs)]
  return np.array([k for k, _ in rows], np.uint64), np.array([h for _, h in rows], np.uint64)


def _assert_equal(got, want, what):
  key, part_hash = got
  wkey, wpart = want
  bad = np.argwhere(part_hash != wpart)
  assert not len(bad), f'{what}: part hashes differ at (env, part) {bad[:6].tolist()}'
  assert (key == wkey).all(), what


def _punch_hole(hs, i):
  """Clears the type of env i's live non-player record in the middle of the prefix, as a despawn of the large-world instance does."""
  objs = state.objs_view(hs.buf['objs'])[i]
  n = int(hs.rec['nobj'][i])
  live = [s for s in range(2, n - 1) if objs[s]['type'] != abi.T_NONE]
  s = live[len(live) // 2]
  objs[s]['type'] = abi.T_NONE
  if 'objmap' in hs.buf:
    cfg = hs.cfg
    hs.buf['objmap'][i].reshape(cfg.W, cfg.H)[objs[s]['x'], objs[s]['y']] = 0
  return s


# ------------------------------------------------------------------ a. the mirror against the body
@pytest.mark.parametrize('geo', [DEFAULT, ODD, SMALL, LARGE], ids=['64x64', '42x30-bytes', '48x40', '256x256-global'])
def test_body_equals_mirror(geo):
  """Part hashes and keys after 0, 1, 8 and 40 steps of a batch whose episodes last 12 steps (auto-resets in between), for every env."""
  from tests.hostsim import fingerprint_build as fb
  seeds = [5, 6, 7, 8, 9]
  hs = _hostsim(seeds, length=12, auto_reset=True, **geo)
  cells = hs.cfg.W * hs.cfg.H
  assert (cells % 8 != 0) == (geo is ODD) and (cells % 16 != 0) == (geo is ODD)
  acts = np.random.RandomState(17).randint(0, 17, size=(41, len(seeds))).astype(np.int32)
  for t in range(41):
    if t in (0, 1, 8, 40):
      _assert_equal(fb.fingerprint(hs), _mirror_rows(hs), f'step {t}')
      for parts in (abi.FP_DYNAMICS, abi.FP_VISIBLE, abi.FP_RNG | abi.FP_IDENT):
        key, _ = fb.fingerprint(hs, parts=parts)
        assert key.tolist() == _mirror_rows(hs, parts)[0].tolist(), (t, parts)
    hs.step(acts[t])
  assert hs.rec['episode'].min() >= 3 and not hs.rec['status'].any()
  if geo is LARGE:   # ... and with a hole in the prefix: rank, not slot number
    before = fb.fingerprint(hs)[1]
    s = _punch_hole(hs, 1)
    objs = state.objs_view(hs.buf['objs'])[1]
    assert s < hs.rec['nobj'][1] - 1 and objs[s]['type'] == abi.T_NONE and objs[s + 1]['type'] != abi.T_NONE
    after = fb.fingerprint(hs)
    _assert_equal(after, _mirror_rows(hs), 'with a hole')
    changed = after[1] != before
    assert changed[1].tolist() == [p == 1 for p in range(abi.FP_PARTS)] and not changed[[0, 2, 3, 4]].any()


def test_key_only_reads_the_parts_it_names():
  """Without part_hash the body computes the named parts only: the key is the same, and equals K over the part hashes."""
  from tests.hostsim import fingerprint_build as fb
  hs = _hostsim([21, 22, 23], **DEFAULT)
  hs.step(np.array([1, 5, 6], np.int32))
  _, part_hash = fb.fingerprint(hs)
  for parts in list(range(1, 8)) + [abi.FP_CLOCK, abi.FP_CHUNKS | abi.FP_IDENT, abi.FP_DYNAMICS, abi.FP_ALL]:
    key = np.zeros(3, np.uint64)
    got = fb.lib().hostsim_fingerprint(fb.C.byref(hs.cfg), fb.C.byref(hs.tb), fb.C.byref(hs.st), None, fb.C.c_uint32(parts), fb._p(key), None)
    assert got == 0
    assert key.tolist() == [state.fingerprint_combine(row, parts) for row in part_hash], parts


# ------------------------------------------------------------------ b. the oracle
@pytest.mark.parametrize('geo', [DEFAULT, ODD], ids=['64x64', '42x30'])
def test_mirror_of_the_oracle_equals_body(geo):
  """fingerprint_host(OracleEnv.snapshot(), lane) against the body on a shared seed and action tape, auto-resets included: the
  VISIBLE parts, CLOCK, RNG and CHUNKS (and the key over them)."""
  from oracle.crafter_oracle import OracleEnv
  from tests.hostsim import fingerprint_build as fb
  seed, length = 31, 25
  hs = _hostsim([seed], length=length, auto_reset=True, **geo)
  orc = OracleEnv(seed=seed, length=length, **geo)
  orc.reset()
  lane = state.seed_lanes([seed])[0]
  acts = np.random.RandomState(3).randint(0, 17, size=60)
  resets = 0
  for t in range(-1, 60):
    if t >= 0:
      hs.step(np.array([acts[t]], np.int32))
      if orc.step(int(acts[t]))[2]:
        orc.reset()
        resets += 1
    key, part_hash = fb.fingerprint(hs, parts=abi.FP_DYNAMICS)
    wkey, want = state.fingerprint_host(orc.snapshot(), lane, abi.FP_DYNAMICS)
    for p in range(6):   # map, objects, player, clock, rng, chunks
      assert int(part_hash[0, p]) == want[p], (t, abi.FP_NAMES[p])
    assert int(key[0]) == wkey, t
  assert resets >= 2


# ------------------------------------------------------------------ c. collisions
def test_no_collisions_over_a_few_thousand_states():
  """36 envs (32 distinct seeds and four twins of the first four on the same tape) x 100 steps, episodes of 40 steps: for each
  part by itself and for the VISIBLE, DYNAMICS and ALL keys, two states have the same hash exactly when the canonical unit
  sequences the hash is built from are equal.  Zero collisions allowed: at 64 bits a few thousand states stay far within that
  (birthday bound 3600^2 / 2^65 < 10^-12)."""
  seeds = list(range(400, 432)) + list(range(400, 404))
  hs = _hostsim(seeds, length=40, auto_reset=True, **DEFAULT)
  acts = np.random.RandomState(23).randint(0, 17, size=(100, 32)).astype(np.int32)
  acts = np.concatenate([acts, acts[:, :4]], axis=1)
  views = {abi.FP_NAMES[p]: 1 << p for p in range(abi.FP_PARTS)}
  views.update(visible=abi.FP_VISIBLE, dynamics=abi.FP_DYNAMICS, all=abi.FP_ALL)
  seen = {name: {} for name in views}   # canonical units -> hash
  states = 0
  for t in range(100):
    hs.step(acts[t])
    for i in range(len(seeds)):
      snap, lane = hs.snapshot(i), hs.rec['seed_lane'][i]
      units = [u.tobytes() for u in state.fingerprint_units(snap, lane)]
      _, hashes = state.fingerprint_host(snap, lane)
      states += 1
      for name, parts in views.items():
        canon = tuple(units[p] for p in range(abi.FP_PARTS) if parts >> p & 1)
        h = hashes[parts.bit_length() - 1] if name in abi.FP_NAMES else state.fingerprint_combine(hashes, parts)
        assert seen[name].setdefault(canon, h) == h
  assert states == 3600
  for name, table in seen.items():
    assert len(set(table.values())) == len(table), f'{name}: {len(table) - len(set(table.values()))} collisions'
  # both directions were exercised: the twins repeat whole states, parts repeat on their own, and the rest is distinct
  assert len(seen['all']) == 3200 and len(seen['dynamics']) == 3200 and 3000 < len(seen['rng']) <= 3200   # (a step may draw nothing)
  assert len(seen['clock']) == 40 and len(seen['ident']) < 200 and len(seen['map']) < 3200 and len(seen['player']) < 3200


# ------------------------------------------------------------------ d. the stand-alone program
def test_body_sanitized_standalone(tmp_path):
  """The body as a stand-alone program under -fsanitize=address,undefined, every buffer of exactly its size: the default
  geometry after 40 steps, the byte path of a 42 x 30 world, a 256 x 256 world with a hole and a row mask.  Same hashes."""
  from tests.hostsim import fingerprint_build as fb
  rs = np.random.RandomState(5)
  for name, geo, mask, parts in (('default', DEFAULT, None, abi.FP_ALL), ('odd', ODD, None, abi.FP_DYNAMICS),
                                 ('large', LARGE, np.array([0, 1, 1], np.uint8), abi.FP_VISIBLE)):
    hs = _hostsim([41, 42, 43], length=15, auto_reset=True, **geo)
    for t in range(40):
      hs.step(rs.randint(0, 17, size=3).astype(np.int32))
    if geo is LARGE:
      _punch_hole(hs, 2)
    fb.dump(hs, tmp_path / f'{name}.blob', parts=parts, mask=mask)
    rows = fb.run_sanitized(tmp_path / f'{name}.blob')
    key, part_hash = fb.fingerprint(hs, parts=parts)
    assert len(rows) == 3
    for i, row in enumerate(rows):
      if mask is not None and not mask[i]:
        assert row is None, name
      else:
        assert row == (int(key[i]), [int(v) for v in part_hash[i]]), (name, i)


# ------------------------------------------------------------------ mask, tail, arguments
def test_body_rows_tail_mask_and_arguments():
  """Five envs (four to a workgroup) with a row mask, written into sentinel-filled buffers inside larger ones: masked rows and
  the words around the buffers stay as they were; what crafter_fingerprint refuses is refused."""
  from tests.hostsim import fingerprint_build as fb
  hs = _hostsim([11, 12, 13, 14, 15], **DEFAULT)
  hs.step(np.array([1, 2, 3, 4, 5], np.int32))
  full_key, full_part = fb.fingerprint(hs)
  sentinel = np.uint64(0x5E5E5E5E5E5E5E5E)
  raw_key, raw_part = np.full(5 + 4, sentinel), np.full(5 * 7 + 4, sentinel)
  key, part = raw_key[2:7], raw_part[2:37].reshape(5, 7)
  mask = np.array([1, 0, 0, 1, 0], np.uint8)
  fb.fingerprint(hs, mask=mask, key=key, part_hash=part)
  for i in range(5):
    if mask[i]:
      assert key[i] == full_key[i] and (part[i] == full_part[i]).all()
    else:
      assert key[i] == sentinel and (part[i] == sentinel).all()
  assert (raw_key[:2] == sentinel).all() and (raw_key[7:] == sentinel).all() and (raw_part[:2] == sentinel).all() and (raw_part[37:] == sentinel).all()
  lib = fb.lib()
  args = (fb.C.byref(hs.cfg), fb.C.byref(hs.tb), fb.C.byref(hs.st), None)
  assert lib.hostsim_fingerprint(*args, fb.C.c_uint32(abi.FP_ALL), None, None) == 1      # both outputs null
  assert lib.hostsim_fingerprint(*args, fb.C.c_uint32(128), fb._p(key), None) == 1          # a bit above 6
  assert lib.hostsim_fingerprint(*args, fb.C.c_uint32(0), fb._p(key), None) == 1            # a key of no part
  assert lib.hostsim_fingerprint(*args, fb.C.c_uint32(0), None, fb._p(part)) == 0           # the part hashes need none
  assert (part == full_part).all()


def test_mirror_arguments():
  hs = _hostsim([3], **SMALL)
  snap, lane = hs.snapshot(0), hs.rec['seed_lane'][0]
  for bad in (0, 128, -1):
    with pytest.raises(ValueError):
      state.fingerprint_host(snap, lane, bad)
  key, hashes = crafter_amd.fingerprint_host(snap, int(lane))
  assert 0 <= key <= U64 and len(hashes) == abi.FP_PARTS and all(0 <= h <= U64 for h in hashes)
  assert crafter_amd.fingerprint_host(snap, np.int64(lane.view(np.int64)))[0] == key   # the lane as int64 bits
  assert state.fingerprint_combine([h - (1 << 64) if h >> 63 else h for h in hashes], abi.FP_ALL) == key   # int64 rows of fingerprint_parts()
  # levels_pick shares mix64: its pinned value (tests/test_levels_host.py holds the rest)
  assert int(state.mix64(np.uint64(1))) == 0x5692161D100B05E5


# ------------------------------------------------------------------ the library
def test_entry_point_declared_listed_and_exported():
  """crafter_fingerprint extends the boundary from a header of its own (include/crafter_hip_fingerprint.h) and lib.EXTENSIONS
  lists it: the core header and lib.SIGNATURES stay the pinned pair tests/test_host_logic.py compares."""
  from crafter_amd import build, lib as hiplib
  header = (ROOT / 'include' / 'crafter_hip_fingerprint.h').read_text()
  assert 'crafter_fingerprint' not in (ROOT / 'include' / 'crafter_hip.h').read_text() and 'crafter_fingerprint' not in hiplib.SIGNATURES
  assert ROOT / 'include' / 'crafter_hip_fingerprint.h' in build.sources()
  path = build.build()
  nm = subprocess.run(['nm', '-D', '--defined-only', str(path)], capture_output=True, text=True, check=True).stdout
  exported = set(re.findall(r'\b(crafter_[a-z_]+)$', nm, re.M))
  assert re.search(r'\bint crafter_fingerprint\(crafter_handle\* h, const uint8_t\* mask, uint32_t parts, uint64_t\* key, '
                   r'uint64_t\* part_hash, void\* stream\);', header)
  assert 'crafter_fingerprint' in exported
  # every extension: its header exists and declares it, the library exports it, load() typed it as the table says
  so = hiplib.load()
  for name, (where, restype, argtypes) in hiplib.EXTENSIONS.items():
    text = re.sub(r'/\*.*?\*/', '', (ROOT / 'include' / where).read_text(), flags=re.S)
    params = re.search(rf'^int {name}\(([^)]*)\)\s*;', text, flags=re.M).group(1).split(',')
    assert len(params) == len(argtypes) and name in exported, name
    for decl, t in zip(params, argtypes):
      assert ('*' in decl) == (t is hiplib.C.c_void_p), (name, decl)
    assert getattr(so, name).restype is restype and list(getattr(so, name).argtypes) == list(argtypes), name
  hip = hiplib.EXTENSIONS['crafter_fingerprint'][2]
  assert len(hip) == 6 and hip[2] is hiplib.C.c_uint32
  assert so.crafter_abi_version() == 7


def test_constants_match_the_c_header(tmp_path):
  """crafter_amd.FP_* against CRAFTER_FP_* as a C compiler reads include/crafter_hip_types.h, through
  include/crafter_hip_fingerprint.h: that header is pedantic C99 by itself."""
  if not shutil.which('gcc'):
    pytest.skip('needs gcc')
  names = ['PARTS', 'MAP', 'OBJECTS', 'PLAYER', 'CLOCK', 'RNG', 'CHUNKS', 'IDENT', 'VISIBLE', 'DYNAMICS', 'ALL']
  header = (ROOT / 'include' / 'crafter_hip_types.h').read_text()
  assert set(re.findall(r'\bCRAFTER_FP_([A-Z]+)\b', header)) == set(names)
  src = tmp_path / 'fp.c'
  src.write_text('#include <stdio.h>\n#include "crafter_hip_fingerprint.h"\nint main(void) {\n' +
                 ''.join(f'  printf("{n} %ld\\n", (long)CRAFTER_FP_{n});\n' for n in names) + '  return 0;\n}\n')
  subprocess.run(['gcc', '-std=c99', '-pedantic', '-Wall', '-Werror', f'-I{ROOT / "include"}', str(src), '-o', str(tmp_path / 'fp')], check=True)
  out = subprocess.run([str(tmp_path / 'fp')], capture_output=True, text=True, check=True).stdout
  assert {k: int(v) for k, v in (line.split() for line in out.splitlines())} == {n: getattr(crafter_amd, f'FP_{n}') for n in names}
  assert crafter_amd.FP_VISIBLE == 7 and crafter_amd.FP_DYNAMICS == 63 and crafter_amd.FP_ALL == 127 and len(abi.FP_NAMES) == abi.FP_PARTS


def test_fingerprint_kernel_budget():
  """No scratch, no spill, eight waves per SIMD: the bar its read-only siblings set (test_legal_kernel_budget)."""
  from crafter_amd import build
  usage = {k: v for k, v in build.resource_usage().items() if k.startswith('crafter_fingerprint_kernel')}
  assert len(usage) == 1, sorted(usage)
  for name, u in usage.items():
    assert u['scratch'] == 0 and u.get('vgpr_spill', 0) == 0, (name, u)
    assert u['occupancy'] >= 8, (name, u)
    assert u['vgprs'] <= 64, (name, u)   # (eight waves per SIMD of 512 registers)
