"""The three ways the library makes the world of one (seed, episode) agree, on the CPU (tests/hostsim/generator_forms_host.cpp):
the world Env.reset leaves in the env's row (reset_body), the pool entry the fused form writes (gen_body: what
crafter_reset_kernel appends) and the pool entry the world pool's seed -> classify -> resolve kernels write.  Equal means:
the material map, the live prefix of the slot table, the MT state and its position, the seen prefix of the chunk order and the
census.  Each form is compared with the oracle elsewhere; this is the direct statement, and the only CPU run of gen_body."""
import subprocess

import numpy as np
import pytest

from tests.hostsim import generator_forms_build as gf
from tests.hostsim.driver import HostSimEnv

# area, view, size, seeds: small on purpose.  42x30 = 1260 cells: one full classification part plus a 236-cell tail that is
# no multiple of 64; 256x256: maps and slot table are generated in place in the pool entry.
SHAPES = {
    '64x64': ((64, 64), (9, 9), (64, 64), [11, 12]),
    '48x40': ((48, 40), (9, 9), (63, 63), [21, 22]),
    '42x30': ((42, 30), (7, 9), (84, 72), [31, 32]),
    '128x128': ((128, 128), (9, 9), (64, 64), [41]),
    '256x256': ((256, 256), (9, 9), (64, 64), [51]),
}
EPISODES = (1, 2, 3)


def make(shape, seeds=None):
  area, view, size, default_seeds = SHAPES[shape]
  return HostSimEnv(seeds or default_seeds, area=area, view=view, size=size)


def assert_same_world(a, b, what):
  for k in gf.FIELDS:
    assert np.array_equal(a[k], b[k]), f'{what}: {k}'


def three_forms(hs, env, episode):
  return gf.reset_world(hs, env, episode), gf.pool_world(hs, env, episode, 'fused'), gf.pool_world(hs, env, episode, 'pipeline')


@pytest.mark.parametrize('shape', list(SHAPES))
def test_three_forms_make_the_same_world(shape):
  hs = make(shape)
  for env in range(hs.cfg.num_envs):
    for episode in EPISODES:
      row, fused, piped = three_forms(hs, env, episode)
      assert len(row['objs']) > 2 and len(row['chunk_order']) >= 1 and row['mt_pos'] != 624, 'an empty world proves nothing'
      assert_same_world(row, fused, f'{shape} env {env} episode {episode}: reset_body / gen_body')
      assert_same_world(row, piped, f'{shape} env {env} episode {episode}: reset_body / pipeline')
  assert not hs.rec['status'].any()


def test_three_forms_on_the_pinned_exp_tie():
  """Episode 10 of seed 7327: a cell at distance 4 on which the noise vanishes, `start > 0.5` decided by exp's last bit."""
  hs = make('64x64', [7327])
  row, fused, piped = three_forms(hs, 0, 10)
  assert_same_world(row, fused, 'reset_body / gen_body')
  assert_same_world(row, piped, 'reset_body / pipeline')


@pytest.mark.parametrize('shape', ['64x64', '42x30', '256x256'])
def test_sanitized_standalone_program(shape, tmp_path):
  """The same three calls under -fsanitize=address,undefined in a program of its own (never loaded into Python), every buffer a
  heap block of exactly its size, every body in "LDS" of exactly its kernel's launch size: it must finish clean, print the same
  line for the three forms, and print what the shared library computes."""
  exe = gf.build_sanitized()
  pairs = [(0, 1), (0, 2)]
  hs = make(shape, SHAPES[shape][3][:1])
  blob = tmp_path / 'forms.blob'
  gf.dump(hs, blob, pairs)
  proc = subprocess.run([str(exe), str(blob)], capture_output=True, text=True)
  assert proc.returncode == 0, proc.stderr[-3000:]
  got = proc.stdout.splitlines()
  want = []
  for env, episode in pairs:
    for form, w in zip(('reset', 'fused', 'pipeline'), three_forms(hs, env, episode)):
      want.append(gf.line(form, env, episode, w))
  assert got == want
  for k in range(len(pairs)):
    tails = {line.split(' ', 1)[1] for line in got[3 * k:3 * k + 3]}
    assert len(tails) == 1, got[3 * k:3 * k + 3]
