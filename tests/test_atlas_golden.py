"""The rule-branch atlas (tests/atlas_cases.py) on the oracle alone, and the oracle against the real reference:
tests/golden/reference_runs/atlas.npz was recorded from the reference playing every case (tools/make_worlds_golden.py: its
generate_world replaced at run time by the authored function).  Data only; replayed here on the CPU, every field at every step."""
import functools

import numpy as np
import pytest

from tests import atlas_cases as ac
from tests.parity import GOLDEN, sha8, state_of_snapshot

FIELDS = ('mat', 'objects', 'inventory', 'achievements', 'misc', 'chunk_order', 'mt_key', 'mt_pos')


@functools.lru_cache(maxsize=None)
def fixture():
  return np.load(GOLDEN / 'reference_runs' / 'atlas.npz')


@pytest.mark.parametrize('geometry', list(ac.GEOMETRIES))
@pytest.mark.parametrize('name', ac.NAMES)
def test_witness_on_the_oracle(name, geometry):
  """Every case reaches its branch at every geometry the atlas is played at, within 64 steps."""
  run = ac.witnessed_run(name, geometry)
  assert 1 <= run.steps <= ac.T and len(ac.CASES[name][1]) <= ac.T and (run.steps == ac.T or run.dones[-1])
  assert not any(run.dones[:-1]), 'a case is compared up to its first done'


@pytest.mark.parametrize('geometry', list(ac.GEOMETRIES))
def test_union_of_the_atlas(geometry):
  """All 22 achievements and all four causes of death, on the oracle alone."""
  reached, deaths = ac.union(geometry)
  assert reached == set(ac.ACHIEVEMENTS) and len(reached) == 22
  assert deaths == {'lava', 'zombie', 'arrow', 'starvation'}


def test_the_mutated_rules_change_a_witness():
  assert 'mine' in ac.witness_changes()   # (iron with the wood pickaxe, at step 14)


@pytest.mark.parametrize('name', ac.NAMES)
def test_oracle_replays_the_reference_fixture(name):
  g = fixture()
  assert list(g['names']) == ac.NAMES and list(g['seeds']) == ac.SEEDS, 'the fixture was recorded from another atlas'
  get = lambda key: g[f'{name}.{key}']
  run = ac.witnessed_run(name)
  assert np.array_equal(get('actions'), ac.tape(name)), 'the fixture was recorded with another tape'
  assert len(get('dones')) == run.steps, 'the reference ended the episode at another step'
  assert np.array_equal(run.frames[0], get('reset_obs'))
  for prefix, snap in (('reset_', run.snapshots[0]), ('final_', run.snapshots[-1])):
    for f, v in state_of_snapshot(snap).items():
      assert np.array_equal(np.asarray(v), get(prefix + f)), f'{prefix}{f}'
  frames = {int(t): fr for t, fr in zip(get('frame_steps'), get('frames'))}
  assert len(frames) == (len(ac.CASES[name][1]) if name in ac.FRAME_CASES else 0)
  for t in range(run.steps + 1):
    s = state_of_snapshot(run.snapshots[t])
    for f in FIELDS:
      assert sha8(s[f]) == get('sha_' + f)[t], f'step {t}: {f}'
    assert sha8(run.frames[t]) == get('obs_sha')[t], f'step {t}: frame'
    if t:
      assert sha8(run.semantic[t].astype(np.uint8)) == get('sem_sha')[t], f'step {t}: semantic'
      assert run.rewards[t - 1] == get('rewards')[t - 1] and run.dones[t - 1] == bool(get('dones')[t - 1]), f'step {t}: reward / done'
      if t - 1 in frames:
        assert np.array_equal(run.frames[t], frames[t - 1]), f'step {t}: pixels'
