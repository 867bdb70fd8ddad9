"""The oracle restatement against the UNTOUCHED reference: the primary pin of oracle/crafter_oracle.py.

The reference's side of every run is stored as digests in tests/golden/reference_runs/oracle_vs_reference.npz (tools/make_reference_runs.py
plays the runs of tests/reference_runs.py on the reference, imported through oracle/reference_harness.py); here the oracle
plays the same runs and every digest must match: obs, reward (value and type), done, info, semantic view, objects, chunk
order and the RNG's key and position after every step."""
import json
import pathlib

import numpy as np
import pytest

from oracle.crafter_oracle import OracleEnv
from tests import reference_runs as rr
from tests import scenarios

GOLDEN = pathlib.Path(__file__).resolve().parent / 'golden'


@pytest.fixture(scope='module')
def ref():
  with np.load(GOLDEN / rr.FIXTURE) as g:
    return {k: g[k] for k in g.files}


def make_oracle(**kw):
  env = OracleEnv(**kw)
  return env, rr.OracleSide(env)


def check_run(ref, name):
  want = ref[f'run_{name}']
  got = np.array(rr.RUNS[name](make_oracle), np.uint64)
  for i, (g, w) in enumerate(zip(got, want)):
    if not np.array_equal(g, w):
      resets = np.flatnonzero(want[:i + 1, 0] == 0)
      episode, steps = len(resets) - 1, int((want[resets[-1]:i + 1, 0] == 1).sum())
      what = [rr.KINDS[int(w[0])][k] for k in range(4) if g[k + 1] != w[k + 1]] if g[0] == w[0] else ['row kind']
      pytest.fail(f'{name}: row {i} (episode {episode}, after {steps} steps) differs from the reference in {what}')
  assert len(got) == len(want), f'{name}: {len(got)} rows, the reference {len(want)}'


@pytest.mark.parametrize('seed', [0, 1, 2, 3])
def test_random_policy_two_episodes(ref, seed):
  check_run(ref, f'random_s{seed}')


@pytest.mark.parametrize('kind', sorted(scenarios.SCENARIOS))
def test_scripted_scenarios(ref, kind):
  check_run(ref, f'scripted_{kind}')


def test_constructor_variants(ref):
  for name in ('variant_area_view_size', 'variant_length_no_reward', 'variant_unbounded_length'):
    check_run(ref, name)


def test_extra_render_calls_consume_night_noise(ref):
  check_run(ref, 'night_renders')


def test_survey_end_to_end_fixture():
  """SURVEY.md App. B 'provisional end-to-end fixtures' (surveyor's own noise restatement)."""
  import hashlib
  o = OracleEnv(seed=0)
  obs = o.reset()
  assert hashlib.sha256(o.mat.tobytes()).hexdigest()[:16] == 'e6448727016242ea'
  assert hashlib.sha256(obs.tobytes()).hexdigest()[:16] == '7ea6d5809711316c'


def test_exp_flavour_is_the_only_difference(ref):
  """VERDICT r3 weak #1b.  The oracle pins worldgen.py:27's exp to the correctly rounded value (oracle/exp_cr.py); the
  reference takes whatever np.exp is on the host -- SVML on AVX-512 hosts, the C library's elsewhere -- and on ~1 world in
  5000 (a structural tie of `start > 0.5` at distance exactly 4 from the player) the flavours decide a material, after
  which every later uniform() of that world shifts.  Seed 7327, episode 10 is such a world: with worldgen's np.exp replaced
  by libm's exp -- the ONLY patch -- the untouched reference produces the oracle's 11 worlds cell for cell, objects included."""
  worlds = rr.worlds(make_oracle, 7327, 11)
  for ep, ((orc_mat, orc_objects), (ref_mat, ref_objects)) in enumerate(zip(worlds, ref['tie_world_libm_exp']), 1):
    assert rr.digest(orc_mat) == ref_mat and orc_objects == ref_objects, f'episode {ep}: reference (libm exp) != oracle'


def test_unpatched_reference_differs_only_where_numpy_exp_misrounds(ref):
  """The same 11 worlds with the reference as it ran on the host that recorded them, whose np.exp flavour is recorded
  with them.  Where numpy's exp rounds the tie cell of episode 10 correctly (non-AVX-512 hosts) everything is equal; where
  it does not (SVML) exactly that world differs -- a dozen cells behind cell (32, 28) in generation order -- and the ten
  others are equal.  Either way the difference is explained by np.exp(-1.638e-16) alone."""
  worlds = rr.worlds(make_oracle, 7327, 11)
  misrounds = bool(ref['host_np_exp_misrounds'])
  for ep, ((orc_mat, orc_objects), ref_mat, ref_objects) in enumerate(
      zip(worlds, ref['tie_world_host_exp_mat'], ref['tie_world_host_exp_objects']), 1):
    if ep == 10 and misrounds:
      bad = np.argwhere(ref_mat != orc_mat)
      # cell (32, 28) is grass either way (with a draw or without one); what differs are cells whose draw came later
      assert 1 <= len(bad) <= 64 and all((x, y) > (32, 28) for x, y in bad.tolist()), (len(bad), bad[:3])
    else:
      assert np.array_equal(ref_mat, orc_mat) and orc_objects == ref_objects, f'episode {ep}'


def test_exp_tie_worlds_of_the_sweep(ref):
  """more than ONE pinned tie world, and a MEASURED rate.  tools/sweep_exp_ties.py swept 400,000 worlds (seeds
  0 .. 99,999, four episodes each, oracle only) for cells at distance exactly 4 from the player whose `start` is non-zero
  rounding dust (< 1e-15): 122 of them, one world in 3,279 -- the first ten are in tests/golden/exp_ties.json.  On every one
  the untouched reference with worldgen's np.exp replaced by the C library's exp (the only patch) produces the oracle's
  world cell for cell, objects included.  The flavour of exp only DECIDES where it rounds exp(-start) to another
  neighbour of 1 than the correctly rounded one -- start around 1.6e-16: ONE of the 400,000 worlds on an AVX-512 host (seed
  20042, episode 1; round 4's "one world in 5000" was the rate of the dust cells, not of the decisions) -- and there the
  unpatched reference differs from the oracle exactly when the recording host's np.exp misrounds the known tie."""
  ties = json.loads((GOLDEN / 'exp_ties.json').read_text())
  assert len(ties['ties']) >= 10 and ties['worlds_swept'] >= 400000
  decisive = ties['decided_differently_by_this_hosts_np_exp']['first']
  assert len(decisive) == ties['decided_differently_by_this_hosts_np_exp']['count'] == 1
  misrounds = bool(ref['host_np_exp_misrounds'])
  cases = ties['ties'] + decisive
  assert len(cases) == len(ref['sweep_ties'])
  for t, (libm_mat, libm_objects, host_mat, host_objects) in zip(cases, ref['sweep_ties']):
    orc_mat, orc_objects = rr.worlds(make_oracle, t['seed'], t['episode'])[-1]
    orc_mat = rr.digest(orc_mat)
    assert orc_mat == libm_mat and orc_objects == libm_objects, f'seed {t["seed"]} episode {t["episode"]}: reference (libm exp) != oracle'
    same = orc_mat == host_mat and orc_objects == host_objects
    assert same == (not (t in decisive and misrounds)), (t, 'unpatched reference', 'equal' if same else 'differs')
