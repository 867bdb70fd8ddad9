"""TEST INFRASTRUCTURE: the reference semantics of a reset into an authored world, stated on the oracle.  OracleEnv keeps world
generation in one overridable method; AuthoredOracle replaces it by "write this map, World.add these objects" built from the
oracle's own _add / _move -- everything around it is OracleEnv.reset (env.py:70-81) unchanged.  tests/golden/authored_*.npz
ties this to the real reference (tools/make_worlds_golden.py replaces its worldgen.generate_world by the same function)."""
import numpy as np

from oracle.crafter_oracle import OracleEnv, PLAYER

FACING = (1, 5)   # classes that keep a facing (player, arrow); the others' is (0, 0)


def clean_world(world, area, n_materials, grass):
  """What the device makes of a world that breaks the rules (include/crafter_hip.h crafter_reset_worlds): -> (mat, objects,
  flagged).  objects: (type, x, y, health, (fx, fy), aux) tuples as given to WorldBank."""
  W, H = area
  mat = np.array(world['mat'], np.int64).copy()
  bad = (mat < 1) | (mat > n_materials)
  flagged = bool(bad.any())
  mat[bad] = grass
  taken, out = {(W // 2, H // 2)}, []
  for k, (typ, x, y, health, (fx, fy), aux) in enumerate(world['objects']):
    if not 1 <= typ <= 6 or not (0 <= x < W and 0 <= y < H) or (typ == PLAYER and k != 0):
      flagged = True
      continue
    if typ in FACING and fx * fx + fy * fy != 1:
      flagged, fx, fy = True, 0, 1
    if typ == PLAYER:
      taken = {(x, y)}
    elif (x, y) in taken:
      flagged = True
      continue
    taken.add((x, y))
    out.append((typ, x, y, health, (fx, fy), aux))
  return mat.astype(np.uint8), out, flagged


class AuthoredOracle(OracleEnv):
  """OracleEnv whose NEXT reset goes into `world` = dict(mat [W][H], objects [(type, x, y, health, (fx, fy), aux)], inventory or
  None); the resets after it generate as usual (an authored world lasts one episode)."""

  def __init__(self, world=None, **kw):
    super().__init__(**kw)
    self.world = world
    self.balance_events = 0   # spawns + despawns by the balance pass so far (the tests' preconditions)
    self.refused_outside = []   # (step, type, tx, ty) of every move tried to a cell outside the map (the rim cases' witness)

  def _try_move(self, slot, px, py, dx, dy, walkable):
    if not self._inside(px + dx, py + dy):
      self.refused_outside.append((self._step, self.otype[slot], px + dx, py + dy))
    return super()._try_move(slot, px, py, dx, dy, walkable)

  def _balance_chunk(self, key):
    before = (len(self.otype), sum(1 for t in self.otype if t))
    super()._balance_chunk(key)
    self.balance_events += before != (len(self.otype), sum(1 for t in self.otype if t))

  def _generate_world(self):
    world, self.world = self.world, None
    if world is None:
      return super()._generate_world()
    self.mat[:] = np.asarray(world['mat'], np.uint8)
    for k, (typ, x, y, health, (fx, fy), aux) in enumerate(world['objects']):
      if typ == PLAYER:
        assert k == 0
        if (x, y) != (self.ox[1], self.oy[1]):
          self._move(1, x, y)
        self.ofx[1], self.ofy[1] = fx, fy
      else:
        if typ not in FACING:
          fx = fy = 0
        self._add(typ, x, y, health, fx, fy, aux)
    if world.get('inventory') is not None:
      self.inv = [int(v) for v in world['inventory']]
