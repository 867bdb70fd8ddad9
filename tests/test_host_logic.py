"""CPU tests of the host side: rule/table compilation, geometry, ABI mirrors, world-seed hash,
and that the product refuses to run without its HIP extension / GPU."""
import ctypes
import pathlib
import re

import numpy as np
import pytest

from crafter_amd import abi, state, tables

ROOT = pathlib.Path(__file__).resolve().parent.parent


def test_rules_compile_matches_data_yaml():
  rules = tables.load_rules()
  R = tables.build_rules(rules)
  assert (R.n_actions, R.n_materials, R.n_items, R.n_achievements) == (17, 12, 16, 22)
  mat = {m: i + 1 for i, m in enumerate(rules['materials'])}
  assert R.walkable_mask == sum(1 << mat[m] for m in rules['walkable'])
  assert R.player_walkable_mask == R.walkable_mask | 1 << mat['lava']
  assert R.arrow_walkable_mask == R.walkable_mask | 1 << mat['lava'] | 1 << mat['water']
  # this reference's data.yaml is NOT upstream's (SURVEY trap 3): the values come from the file
  assert R.collect[mat['tree']].leaves == mat[rules['collect']['tree']['leaves']]
  table = R.place[list(rules['place']).index('table')]
  assert table.uses.n == 1 and table.uses.amount[0] == rules['place']['table']['uses']['wood']
  grass = R.collect[mat['grass']]
  assert grass.probability == rules['collect']['grass']['probability'] and grass.receive.n == 1
  kinds = [R.action_kind[i] for i in range(17)]
  assert kinds[:7] == [abi.A_NOOP] + [abi.A_MOVE] * 4 + [abi.A_DO, abi.A_SLEEP]
  assert kinds[7:11] == [abi.A_PLACE] * 4 and kinds[11:] == [abi.A_MAKE] * 6


def test_runtime_rule_mutation_like_run_random():
  """run_random.py:21-22 mutates constants.items['health'] before building the Env."""
  rules = tables.load_rules()
  rules['items']['health'] = {'max': 5, 'initial': 5}
  R = tables.build_rules(rules)
  assert R.item_max[R.item_health] == 5 and R.item_init[R.item_health] == 5


def test_missing_rule_name_fails_loudly():
  rules = tables.load_rules()
  rules['achievements'] = [a for a in rules['achievements'] if a != 'wake_up']
  with pytest.raises(KeyError):
    tables.build_rules(rules)


def test_geometry_matches_reference_arithmetic():
  cfg, geo = tables.make_config(4, tables.load_rules())
  assert (cfg.unit_x, cfg.unit_y) == (7, 7) and (cfg.local_gw, cfg.local_gh) == (9, 7)
  assert (cfg.item_gw, cfg.item_gh) == (9, 2) and (cfg.border_x, cfg.border_y) == (0, 0)
  assert (cfg.icon_w, cfg.digit_w) == (5, 4) and cfg.update_dist == 18
  assert geo['item_pos'][10].tolist() == [7, 7, 9, 9]   # item 10 -> cell (1, 1): int(7+0.7), int(7+2.8)
  cfg2, _ = tables.make_config(1, tables.load_rules(), size=(512, 512))
  assert (cfg2.unit_x, cfg2.icon_w, cfg2.digit_w, cfg2.border_x) == (56, 44, 33, 4)


def test_atlas_uses_pillow_nearest_columns():
  """NEAREST 16->7 picks source columns [1,3,5,7,10,12,14], not floor((i+.5)*16/7)."""
  rules, tex = tables.load_rules(), tables.load_textures()
  cfg, geo = tables.make_config(1, rules)
  at = tables.build_atlas(rules, tex, geo)
  grass = at['atlas'][at['tex_tile'][1 + rules['materials'].index('grass')]:][:7 * 7 * 4].reshape(7, 7, 4)
  src = tex['grass'].transpose(1, 0, 2)
  cols = [1, 3, 5, 7, 10, 12, 14]
  assert np.array_equal(grass[..., :3], src[cols][:, cols])
  assert at['tex_alpha'][1 + rules['materials'].index('grass')] == 0       # RGB png -> opaque copy
  assert at['tex_alpha'][abi.TEX_ZOMBIE] == 1


def test_daylight_and_vignette_tables():
  d = tables.daylight_table(400)
  assert abs(d[0] - 0.79693) < 1e-5 and (d[148:273] < 0.5).all() and d[147] >= 0.5 and d[273] >= 0.5
  v = tables.vignette_table((63, 49))
  assert v.shape == (63, 49) and v[31, 24] == 0.0 and abs(v[0, 0] - (1 - np.exp(-4.0))) < 1e-15


def test_struct_mirrors_and_library_exports():
  from tests.hostsim import driver
  lib = driver.lib()   # raises on any sizeof mismatch between abi.py and the C++ structs
  assert abi.REC_DTYPE.itemsize == abi.SIZES['EnvRec']
  # every function declared in include/crafter_hip.h is exported by the built HIP library
  header = (ROOT / 'include' / 'crafter_hip.h').read_text()
  declared = sorted(set(re.findall(r'\b(crafter_[a-z_]+)\s*\(', header)))
  from crafter_amd import build, lib as hiplib
  path = build.build()
  so = ctypes.CDLL(str(path))
  missing = [n for n in declared if not hasattr(so, n)]
  assert not missing, missing
  assert set(hiplib.EXPORTS) <= set(declared)
  loaded = hiplib.load()
  assert loaded.crafter_abi_version() == 7


def test_world_seed_hash_matches_cpython():
  """env.py:74: hash((seed, episode)) % (2**31 - 1), restated on the device from CPython's tuplehash."""
  from tests.hostsim import driver
  lib = driver.lib()
  cases = [(0, 1), (1, 1), (12345, 3), (2 ** 31 - 2, 7), (2 ** 40 + 3, 2), (-5, 9), (-1, 1), ('abc', 4), ((1, 2), 5)]
  for seed, ep in cases:
    lane = int(state.seed_lanes([seed])[0])
    assert lib.hostsim_world_seed(lane, ep) == hash((seed, ep)) % (2 ** 31 - 1), (seed, ep)
  assert hash((0, 1)) % (2 ** 31 - 1) == 1256191933   # SURVEY A.6 probe value (CPython 3.10)


def test_product_refuses_to_run_without_gpu():
  import torch
  if torch.cuda.is_available():
    pytest.skip('GPU present')
  import crafter_amd
  with pytest.raises(crafter_amd.CrafterDeviceError):
    crafter_amd.BatchedEnv(2)
  with pytest.raises(crafter_amd.CrafterDeviceError):
    crafter_amd.Env(seed=0)


def test_product_never_imports_oracle_or_hostsim():
  for p in (ROOT / 'crafter_amd').glob('*.py'):
    text = p.read_text()
    assert 'oracle' not in text.replace('the oracle', '').replace("oracle's", '') or p.name == 'state.py', p
    assert 'hostsim' not in text, p


def test_stats_rows_match_reference_statsrecorder_layout():
  """recorder.py:53-66: {'length', 'reward' (rounded to .1), 'achievement_<name>'...} per finished episode,
  rebuilt from the device-side terminal record; checked against the oracle driven like StatsRecorder."""
  from crafter_amd.recorder import episode_rows
  from oracle.crafter_oracle import OracleEnv
  from tests.hostsim.driver import HostSimEnv
  seeds, length = [3, 4, 5], 35
  hs = HostSimEnv(seeds, auto_reset=True, length=length, pool=True)
  orcs = [OracleEnv(seed=s, length=length) for s in seeds]
  hs.reset()
  for o in orcs:
    o.reset()
  acc = [[0, 0.0] for _ in seeds]
  rs = np.random.RandomState(2)
  got, want = [], []
  for t in range(120):
    acts = rs.randint(0, 17, size=len(seeds))
    _, _, done = hs.step(acts)
    for i, o in enumerate(orcs):
      _, _, d, info = o.step(int(acts[i]))
      acc[i][0] += 1
      acc[i][1] += info['reward']
      if d:
        row = {'length': acc[i][0], 'reward': round(acc[i][1], 1)}
        row.update({f'achievement_{k}': v for k, v in info['achievements'].items()})
        want.append(row)
        acc[i] = [0, 0.0]
        o.reset()
      assert bool(done[i]) == bool(d)
    idx = np.nonzero(done)[0]
    got += episode_rows(hs.terminal[idx], list(hs.rules_dict['achievements']))
  assert len(want) >= 9 and got == want


def test_step_kernel_stays_out_of_scratch():
  """The latency-critical kernels must not spill: a single non-inlined helper pushes the whole Env
  object to scratch memory (seen twice during development: +5x HBM traffic, +30% kernel time).  And every kernel keeps
  the register budget its residency was designed for (waves per SIMD; VERDICT r5 #7: a compiler bump must fail HERE, not
  in a benchmark): the resident rollout kernel of the default instance is bounded to 80 VGPRs by hand (six workgroups per
  CU, csrc/crafter_rollout.hip) and spills the day the allocator wants more."""
  from crafter_amd import build
  usage = build.resource_usage()
  # kernel -> (least waves per SIMD, may spill).  One workgroup of 256 threads is one wave per SIMD: six resident step
  # workgroups per CU need occupancy >= 6; the rule kernel (one wave per env, sixteen envs per CU) >= 4; the frame kernel 8.
  budget = {
      'crafter_step_kernel<1,1,1>': (6, False), 'crafter_step_kernel<1,1,0>': (6, False), 'crafter_step_kernel<1,0,0>': (5, False),
      # worlds whose maps and slot table stay in global memory (BASELINE configs[3]): 15 KB of LDS, so registers decide -- six waves per
      # SIMD, WITHOUT a spilled vector register (79 VGPRs since the batched spawn-cell search is off: a kernel of this instance that
      # spilled both vector and scalar registers was miscompiled in round 6)
      'crafter_step_kernel<0,0,0>': (6, False), 'crafter_step_kernel<0,2,1>': (6, False), 'crafter_step_wide_kernel': (6, False), 'crafter_render_kernel': (4, False),
      'crafter_step_early_kernel': (6, False),
      'crafter_rollout_kernel<1,1,1>': (6, False), 'crafter_rollout_kernel<1,1,0>': (6, False), 'crafter_rollout_kernel<1,0,0>': (3, False),
      'crafter_rollout_kernel<0,0,0>': (4, False), 'crafter_rollout_kernel<0,2,1>': (6, False), 'crafter_rules_kernel': (4, False),
      'crafter_frame_kernel': (7, False),   # (55 VGPRs; 101 SGPRs since the /255 table is read through a pointer: seven waves per SIMD by the scalar file)
      # the inline-regeneration kernels find their queue empty all but always: bounded so that the empty look does not wait
      # for half a CU's registers, and allowed to spill on the rare path for it
      'crafter_requeue_reset_kernel': (5, True), 'crafter_requeue_rollout_kernel': (4, True),
      # the world pool's kernels run BESIDE six step workgroups per CU: their waves must fit what those leave of a SIMD's registers
      # (512 - 6 x 64 = 128), and they never spill in their loops
      # (round 6: the default instance's workgroup is 20 LDS granules, six of them leave room for a classification workgroup -- which
      # is bounded to the 80 VGPRs six early-frame step waves leave of a SIMD and spills two dozen for it: profiles/r6_diet_ab.txt)
      'crafter_gen_seed_kernel<1>': (8, False), 'crafter_gen_classify_kernel<1>': (6, 24), 'crafter_gen_resolve_kernel<1>': (4, None),
  }
  for k, (occ, may_spill) in budget.items():
    assert k in usage, (k, sorted(usage))
    if may_spill is False:
      assert usage[k]['scratch'] == 0 and usage[k]['vgpr_spill'] == 0, (k, usage[k])
    elif may_spill is None:   # (a few bytes of scratch for an out-of-line call's frame: no register spilled)
      assert usage[k]['vgpr_spill'] == 0 and usage[k]['scratch'] <= 128, (k, usage[k])
    elif may_spill is not True:   # at most this many spilled registers
      assert usage[k]['vgpr_spill'] <= may_spill and usage[k]['scratch'] <= 4 * may_spill + 16, (k, usage[k])
    assert usage[k]['occupancy'] >= occ, (k, usage[k])
  for k in ('crafter_gen_classify_kernel<1>', 'crafter_gen_resolve_kernel<1>'):
    assert usage[k]['vgprs'] <= 128, (k, usage[k])


def test_build_reads_one_unit_table():
  """build.UNITS is the one list of translation units: every csrc/*.hip is on it, sources() (the staleness check and the
  source hash) sees every unit and every header, and resource_usage() hands each caller a dictionary of its own."""
  from crafter_amd import build
  csrc = build.ROOT / 'csrc'
  units = {name for name, _ in build.UNITS}
  assert {p.name for p in csrc.glob('*.hip')} <= units
  srcs = set(build.sources())
  assert {csrc / name for name in units} <= srcs
  assert set(csrc.glob('*.hpp')) <= srcs
  a, b = build.resource_usage(), build.resource_usage()
  assert a == b and a is not b
  assert all(a[k] is not b[k] for k in a)


def test_compiled_in_default_rules_are_current():
  """csrc/default_rules.inc (the step kernel's compile-time rules) is what tables.build_rules makes of data/rules.json."""
  import importlib.util
  import pathlib
  root = pathlib.Path(__file__).resolve().parent.parent
  spec = importlib.util.spec_from_file_location('bake_default_rules', root / 'tools' / 'bake_default_rules.py')
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  assert (root / 'crafter_amd' / 'csrc' / 'default_rules.inc').read_text() == mod.render()


def test_reference_gym_ids_are_opt_in():
  """crafter/__init__.py:4-17 registers CrafterReward-v1 / CrafterNoReward-v1 at import; here that is an explicit call (a
  process may import both packages).  Without gym it raises ImportError like gym.make itself would."""
  import crafter_amd
  try:
    import gym  # noqa: F401
  except ImportError:
    with pytest.raises(ImportError):
      crafter_amd.register_reference_ids()
  else:
    assert set(crafter_amd.register_reference_ids(force=True)) == {'CrafterReward-v1', 'CrafterNoReward-v1'}


def test_exchange_record_layout_is_aligned_and_viewable():
  """crafter_amd.dist: the packed (obs, reward, done) record of StepExchange -- offsets multiples of 256, views typed and
  shaped like BatchedEnv's outputs (what step(out=...) requires), no copies."""
  import torch
  from crafter_amd import dist as cdist
  slot = cdist._Slot(512, 8, (64, 64, 3), 'cpu')
  assert slot.off_reward % 256 == 0 and slot.off_done % 256 == 0 and slot.record_bytes % 256 == 0
  assert slot.record_bytes == 512 * 12288 + 2048 + 512
  obs, reward, done = slot.outputs()
  assert obs.shape == (512, 64, 64, 3) and obs.dtype == torch.uint8 and obs.data_ptr() == slot.local.data_ptr()
  assert reward.shape == (512,) and reward.dtype == torch.float32 and reward.data_ptr() == slot.local.data_ptr() + slot.off_reward
  assert done.shape == (512,) and done.dtype == torch.uint8 and done.data_ptr() == slot.local.data_ptr() + slot.off_done
  g_obs, g_rew, g_done = slot._views(slot.gathered, (8,))
  assert g_obs.shape == (8, 512, 64, 64, 3) and g_obs.data_ptr() == slot.gathered.data_ptr()
  assert g_rew.shape == (8, 512) and g_done.shape == (8, 512)


def test_c_header_is_self_contained_c99(tmp_path):
  """include/crafter_hip.h (+ crafter_hip_types.h) compiles as pedantic C99 and the C driver of the boundary links
  against the library (no GPU: it is only built here; tests/test_gpu_c_boundary.py runs it)."""
  import shutil
  import pytest
  from tests import c_boundary
  if not shutil.which('gcc') or not pathlib.Path('/opt/rocm/include/hip/hip_runtime_api.h').exists():
    pytest.skip('needs gcc and the HIP runtime headers')
  exe = c_boundary.compile_c(tmp_path / 'boundary_test')
  assert exe.exists()
  cfg = c_boundary.write_tables(tmp_path / 'tables.bin')
  assert cfg.n_daylight == 10002 and (tmp_path / 'tables.bin').stat().st_size > 100000


def test_python_mirror_matches_the_c_header():
  """crafter_amd/abi.py (and lib.HostTablesC) against include/crafter_hip_types.h as a C compiler reads it: sizeof of every
  struct, offset and size of every field, the number of fields (tests/abi_layout.py: a field missing on either side does not
  compile) and every constant and enum value, under the names both sides give them."""
  import shutil
  import pytest
  from tests import abi_layout
  if not shutil.which('gcc'):
    pytest.skip('needs gcc')
  sizes, fields, values = abi_layout.header_report()
  layouts = abi_layout.python_layouts()
  assert set(sizes) == set(layouts) and len(fields) == sum(len(f) for _, f in layouts.values())
  for struct, (size, flds) in layouts.items():
    assert sizes[struct] == size, (struct, sizes[struct], size)
    for name, offset, fsize, _ in flds:
      assert fields[struct, name] == (offset, fsize), (struct, name, fields[struct, name], (offset, fsize))
  mine = abi_layout.python_values()
  assert set(mine) == abi_layout.header_value_names(), set(mine) ^ abi_layout.header_value_names()
  assert mine == values, {n: (mine[n], values[n]) for n in mine if mine[n] != values[n]}
  assert len(mine) == 7 + 6 + 7 + 16 + 7 + 2   # T_*, A_*, ST_*, TEX_*, MAX_*, MT_N and CHUNK


def test_daylight_table_grows_ahead_of_the_longest_episode():
  """BatchedEnv._grow_daylight (Env(length=None), env.py:29): the host-side policy alone, on a stand-in for the device --
  the bound kept between calls is conservative, the step counters are read back only when it nears the end of the table,
  the table grows (on every handle over the state) only when an episode really is that long, and what it grows by is the
  reference's own expression (env.py:135-139), entry for entry."""
  import types
  import torch
  from crafter_amd import batched, tables

  calls = []

  class Lib:
    def crafter_extend_daylight(self, ptr, table, n):
      calls.append((ptr, int(n)))
      return 0

  def handle(n):
    h = types.SimpleNamespace(ptr=object(), cfg=types.SimpleNamespace(n_daylight=n), tables=types.SimpleNamespace(daylight=None))
    h.check = lambda rc: None
    return h

  env = object.__new__(batched.BatchedEnv)
  n0 = 1200
  env.cfg = types.SimpleNamespace(n_daylight=n0, length=0)
  env.tables = types.SimpleNamespace(daylight=tables.daylight_table(n0))
  env._native, env._aux = handle(n0), {(96, 96): handle(n0)}
  env._lib, env.device = Lib(), torch.device('cpu')
  env._off = {'step': 0}
  env._rec_i32 = torch.zeros((4, 1), dtype=torch.int32)
  env._unbounded, env._step_bound = True, 0
  import contextlib
  orig = torch.cuda.device
  torch.cuda.device = lambda d: contextlib.nullcontext()
  try:
    for t in range(1, 1300):   # short episodes: the counters stay small, the table must not grow (one look at the device near call 1192)
      env._rec_i32[:, 0] = t % 150
      env._grow_daylight(1)
    assert calls == [] and env.cfg.n_daylight == n0 and env._step_bound < 400
    for t in range(1, 1400):   # one env never dies
      env._rec_i32[0, 0] = t
      env._grow_daylight(1)
      assert int(env._rec_i32.max()) + 2 < env.cfg.n_daylight, t
    assert len(calls) == 2 and calls[0][1] == calls[1][1] == env.cfg.n_daylight > 2 * n0 - 1   # both handles, once
    assert env._native.cfg.n_daylight == env._aux[(96, 96)].cfg.n_daylight == env.cfg.n_daylight
    assert np.array_equal(env.tables.daylight, tables.daylight_table(env.cfg.n_daylight))
    env._grow_daylight(5000)   # (the first growth adds at least tables.UNBOUNDED_DAYLIGHT entries: room enough)
    assert len(calls) == 2
    env._grow_daylight(200000)   # a rollout longer than what is left of the table
    assert env.cfg.n_daylight > int(env._rec_i32.max()) + 5000 + 200000 and len(calls) == 4
  finally:
    torch.cuda.device = orig


# ------------------------------------------------------------------ the Python binding (crafter_amd/lib.py, batched.py)
_C_CLASS = {'int': 'i32', 'int32_t': 'i32', 'uint32_t': 'u32', 'int64_t': 'i64', 'uint64_t': 'u64'}
_CTYPES_CLASS = {ctypes.c_int: 'i32', ctypes.c_int32: 'i32', ctypes.c_uint32: 'u32', ctypes.c_int64: 'i64', ctypes.c_uint64: 'u64'}


def _header_prototypes():
  """include/crafter_hip.h -> {function: (class of the return value, [class of each parameter])}, whole parameter lists
  (several span lines); classes: pointer (any pointer or array), i32, u32, i64, u64, none (void), string (const char*)."""
  text = re.sub(r'/\*.*?\*/', '', (ROOT / 'include' / 'crafter_hip.h').read_text(), flags=re.S)

  def cls(decl, ret=False):
    decl = decl.strip()
    if ret and decl == 'void':
      return 'none'
    if ret and re.fullmatch(r'const\s+char\s*\*', decl):
      return 'string'
    if '*' in decl or '[' in decl:
      return 'pointer'
    return _C_CLASS[decl.replace('const ', '').split()[0]]

  protos = {}
  for ret, name, params in re.findall(r'^((?:const\s+)?\w+\s*\**)\s*(crafter_\w+)\s*\(([^)]*)\)\s*;', text, flags=re.M):
    params = [] if params.strip() == 'void' else params.split(',')
    protos[name] = (cls(ret, ret=True), [cls(p) for p in params])
  return protos


def _ctypes_class(t):
  if t is None:
    return 'none'
  if t is ctypes.c_char_p:
    return 'string'
  if t is ctypes.c_void_p or issubclass(t, (ctypes._Pointer, ctypes.Array)):
    return 'pointer'
  return _CTYPES_CLASS[t]


def _signature_mismatches(signatures):
  protos = _header_prototypes()
  bad = sorted(set(protos) ^ set(signatures))
  for name in set(protos) & set(signatures):
    restype, argtypes, _ = signatures[name]
    mine = (_ctypes_class(restype), [_ctypes_class(t) for t in argtypes])
    if mine != protos[name]:
      bad.append((name, mine, protos[name]))
  return bad


def test_signature_table_matches_the_c_header():
  """lib.SIGNATURES against every prototype of include/crafter_hip.h: the same set of names, and for each the class of the
  return value and of every parameter, in order.  (The check itself is checked: a table with one i32 read as a pointer, one
  parameter short or one name short does not pass.)"""
  from crafter_amd import lib as hiplib
  protos = _header_prototypes()
  assert len(protos) == 40 and protos['crafter_abi_version'] == ('i32', []) and protos['crafter_last_error'] == ('string', ['pointer'])
  assert protos['crafter_set_levels'] == ('i32', ['pointer'] * 4 + ['i32', 'u64', 'pointer'])   # (a list over two lines)
  assert protos['crafter_struct_sizes'] == ('none', ['pointer']) and protos['crafter_debug_eval'][1][0] == 'i32'
  assert _signature_mismatches(hiplib.SIGNATURES) == []
  assert hiplib.EXPORTS == list(hiplib.SIGNATURES)
  restype, argtypes, optional = hiplib.SIGNATURES['crafter_step_envs']
  for wrong in ((restype, [ctypes.c_void_p] * 8, optional), (restype, argtypes[:-1], optional), (None, argtypes, optional)):
    assert [b[0] for b in _signature_mismatches({**hiplib.SIGNATURES, 'crafter_step_envs': wrong})] == ['crafter_step_envs']
  assert _signature_mismatches({k: v for k, v in hiplib.SIGNATURES.items() if k != 'crafter_reseed'}) == ['crafter_reseed']
  # optional: exactly what an older ABI may lack -- the daylight growth, the exchange family and the twelve newer entry points
  optional = {n for n, s in hiplib.SIGNATURES.items() if s[2]}
  assert {n for n in optional if 'exchange' in n} == {n for n in hiplib.SIGNATURES if 'exchange' in n} and len(optional) == 1 + 6 + 12
  assert not optional & {'crafter_create', 'crafter_step', 'crafter_step_n', 'crafter_reset', 'crafter_render', 'crafter_last_error'}
  so = hiplib.load()   # what load() set is the table
  for name, (restype, argtypes, _) in hiplib.SIGNATURES.items():
    assert getattr(so, name).restype is restype and list(getattr(so, name).argtypes) == list(argtypes), name


def test_require_names_symbol_and_feature():
  import types
  from crafter_amd import lib as hiplib
  stub = types.SimpleNamespace(crafter_step=len)
  assert hiplib.require(stub, 'crafter_step', 'stepping') is len
  with pytest.raises(hiplib.CrafterLibError) as e:
    hiplib.require(stub, 'crafter_reseed', 'level selection')
  assert 'crafter_reseed' in str(e.value) and 'level selection' in str(e.value) and 'older build' in str(e.value)


def test_host_index_checks_without_a_device():
  import torch
  from crafter_amd.batched import BatchedEnv
  check = BatchedEnv._host_index
  a = check([], 4, 'idx', unique=True)
  assert a.dtype == np.int64 and a.size == 0
  for idx in ([3, 0, 2], torch.tensor([3, 0, 2]), np.array([3, 0, 2], np.int16), np.array([[3], [0], [2]])):
    a = check(idx, 4, 'idx', unique=True)
    assert a.dtype == np.int64 and a.tolist() == [3, 0, 2]
  assert check([1, 1, 3], 4, 'idx').tolist() == [1, 1, 3]   # a source may be copied twice
  for idx, unique in (([0.0, 1.0], False), ([0, -1], False), ([0, 4], False), ([1, 1, 3], True), (torch.tensor([2, 2]), True),
                      (torch.tensor([0.5]), False), (np.array([7], np.int16), False)):
    with pytest.raises(ValueError) as e:
      check(idx, 4, 'dst', unique=unique)
    assert 'dst' in str(e.value)


def test_episodes_arg_checks_without_a_device():
  import torch
  from crafter_amd.batched import BatchedEnv
  check = BatchedEnv._episodes_arg
  assert check(None, 4, 'the batch has 4 envs') is None
  for given, want in ((2, [2, 2, 2, 2]), ([1, 2, 3, BatchedEnv.MAX_EPISODE], [1, 2, 3, 2 ** 31 - 3]), (torch.tensor([4, 3, 2, 1]), [4, 3, 2, 1])):
    eps = check(given, 4, 'the batch has 4 envs')
    assert eps.dtype == np.int32 and eps.tolist() == want
  for episodes in ([1, 2, 3], 0, [1, 1, 0, 1], -1, 2 ** 31 - 2, [1.5, 1, 1, 1], [[1, 2], [3, 4], [5, 6]], 1.0):
    with pytest.raises(ValueError):
      check(episodes, 4, 'the table has 4 levels')
  for episodes in ([1, 2, 3], [[1, 2], [3, 4], [5, 6]]):
    with pytest.raises(ValueError, match='the table has 4 levels'):
      check(episodes, 4, 'the table has 4 levels')
