"""The legal-action mask (BatchedEnv.legal_actions, include/crafter_hip.h crafter_legal_actions) restated in plain Python from an
OracleEnv -- mat, _cell, objects(), inv, sleeping and the rules tables --, the tapes the legal-action tests share and the
poked edge states.

legal uint8 [n_actions], in rules['actions'] order: 1 iff Player.update (objects.py:99-131) with that action passes every guard
of the action's branch on the state as it stands."""
import numpy as np

from tests import scenarios
from tests import symbolic_ref as sr

PLAYER, COW, ZOMBIE, SKELETON, ARROW, PLANT = 1, 2, 3, 4, 5, 6
DIRS = dict(left=(-1, 0), right=(1, 0), up=(0, -1), down=(0, 1))

# (kind, seed, steps, area, steps before which every live plant's `grown` is set to 301), as tests/symbolic_ref.py has them
CASES = {
    'builder': ('builder', 3, 400, (64, 64), ()),
    'sleeper': ('sleeper', 7, 300, (64, 64), ()),
    'fighter': ('fighter', 5, 200, (16, 16), ()),
    'planter': ('planter', 5, 400, (64, 64), (100, 200)),
}

# No tape ever has the player at the world's border with a table nearby, so World.nearby's numpy slices (empty at x == 0 or
# y == 0, clipped at the far edges) are shown on poked states: the reset state of EDGE_SEED's 16 x 16 world with the RICH
# inventory, the player's record put on a border cell, a table on its first in-world neighbour (in left, right, up, down
# order) and a furnace on its second, once facing out of the world and once facing its last in-world neighbour.  Observed
# only, never stepped: writing materials directly leaves the chunk census behind.
EDGE_SEED, EDGE_AREA = 5, (16, 16)
EDGE_POSITIONS = ((0, 5), (5, 0), (0, 0), (15, 5), (5, 15), (15, 15))


def edge_states(area=EDGE_AREA, positions=EDGE_POSITIONS):
  """-> [dict(pos, facing, table, furnace, outward)]: two states per position (twelve by default)."""
  W, H = area
  out = []
  for x, y in positions:
    dirs = list(DIRS.values())
    inward = [d for d in dirs if 0 <= x + d[0] < W and 0 <= y + d[1] < H]
    outward = [d for d in dirs if d not in inward]
    table, furnace = ((x + d[0], y + d[1]) for d in inward[:2])
    for facing, is_out in ((outward[0], True), (inward[-1], False)):
      out.append(dict(pos=(x, y), facing=facing, table=table, furnace=furnace, outward=is_out))
  return out


def tape(case):
  kind, seed, steps, area, poke = CASES[case]
  acts, gifts = scenarios.SCENARIOS[kind](steps, seed)
  return acts, gifts, seed, area, poke


def _has(orc, amounts):
  items = orc.t.item_id
  return all(orc.inv[items[k]] >= v for k, v in amounts.items())


def legal_of(orc):
  """-> uint8 [n_actions] of the oracle's current state."""
  t, rules = orc.t, orc.t.rules
  W, H = orc._area
  objs = orc.objects()
  assert objs[0][0] == PLAYER
  _, px, py, _, fx, fy, _ = objs[0]
  by_cell = {(o[1], o[2]): o for o in objs}
  tx, ty = px + fx, py + fy
  material, slot = orc._cell(tx, ty)
  name = t.materials[material - 1] if material else None
  energy = t.item_id['energy']
  tired = orc.inv[energy] < t.item_max[energy]
  awake = not (orc.sleeping and tired)
  # World.nearby(pos, 1) with numpy's slices (engine.py:95-98)
  nearby = {t.materials[m - 1] for m in set(orc.mat[px - 1: px + 2, py - 1: py + 2].flatten().tolist()) if m}
  out = np.zeros(len(t.actions), np.uint8)
  for a, action in enumerate(t.actions):
    if action == 'noop':
      ok = True
    elif action.startswith('move_'):
      dx, dy = DIRS[action[5:]]
      m, s = orc._cell(px + dx, py + dy)
      ok = awake and orc._inside(px + dx, py + dy) and not s and m in t.player_walkable
    elif action == 'do' and slot:
      typ, aux = by_cell[(tx, ty)][0], by_cell[(tx, ty)][6]
      ok = awake and (typ in (ZOMBIE, SKELETON, COW) or (typ == PLANT and aux > 300))
    elif action == 'do':
      info = rules['collect'].get(name)
      ok = awake and (name == 'water' or bool(info and _has(orc, info['require'])))
    elif action == 'sleep':
      ok = not orc.sleeping and tired
    elif action.startswith('place_'):
      info = rules['place'][action[6:]]
      ok = awake and not slot and name in info['where'] and _has(orc, info['uses'])
    elif action.startswith('make_'):
      info = rules['make'][action[5:]]
      ok = awake and all(u in nearby for u in info['nearby']) and _has(orc, info['uses'])
    else:
      raise ValueError(action)
    out[a] = ok
  return out


def oracle_run(case, area=None, view=(9, 9), size=(64, 64), steps=None, rules=None):
  """-> (a reset OracleEnv for the case, its actions, its gifts {step: {item: amount}}, its poke steps): the caller applies
  gifts[t] and the poke to both sides before step t (symbolic_ref.gift_oracle / poke_oracle on this one)."""
  from oracle.crafter_oracle import OracleEnv
  acts, gifts, seed, case_area, poke = tape(case)
  orc = OracleEnv(area=area or case_area, view=view, size=size, seed=seed, rules=rules)
  orc.reset()
  return orc, acts[:steps], gifts, poke


def oracle_trace(case, **kw):
  """-> legal u8 [T + 1, n_actions] of the case on the oracle: after reset, then after every step."""
  orc, acts, gifts, poke = oracle_run(case, **kw)
  out = [legal_of(orc)]
  for t, a in enumerate(acts):
    if t in gifts:
      sr.gift_oracle(orc, gifts[t])
    if t in poke:
      sr.poke_oracle(orc)
    orc.step(int(a))
    out.append(legal_of(orc))
  return np.stack(out)


# ------------------------------------------------------------------ the edge states, on each kind of state
def poke_edge_oracle(orc, edge):
  """The edge state written into OracleEnv `orc` as it stands (the player's slot id moves with its record)."""
  sr.gift_oracle(orc, scenarios.RICH)
  (x, y), (fx, fy) = edge['pos'], edge['facing']
  orc.objmap[orc.ox[1], orc.oy[1]] = 0
  orc.objmap[x, y] = 1
  orc.ox[1], orc.oy[1], orc.ofx[1], orc.ofy[1] = x, y, fx, fy
  orc.mat[edge['table']] = orc.t.mat_id['table']
  orc.mat[edge['furnace']] = orc.t.mat_id['furnace']


def edge_oracle(edge):
  """-> a fresh OracleEnv in the edge state."""
  from oracle.crafter_oracle import OracleEnv
  orc = OracleEnv(area=EDGE_AREA, seed=EDGE_SEED)
  orc.reset()
  poke_edge_oracle(orc, edge)
  return orc


def edge_trace():
  return np.stack([legal_of(edge_oracle(e)) for e in edge_states()])


def edge_arrays(edge, rules, mat, objs, inv, objmap=None):
  """The edge state written into one env's arrays as they stand (for edge_states(): the reset state of EDGE_SEED's world):
  mat u8 [W, H], objs (a crafter_amd.state.objs_view row), inv (the record's inventory) and, where the cell -> slot map is
  state, objmap u16 [W, H], in which the player's slot id moves with its record."""
  materials, items = list(rules['materials']), list(rules['items'])
  (x, y), (fx, fy) = edge['pos'], edge['facing']
  if objmap is not None:
    objmap[int(objs['x'][1]), int(objs['y'][1])] = 0
    objmap[x, y] = 1
  objs['x'][1], objs['y'][1], objs['fx'][1], objs['fy'][1] = x, y, fx, fy
  mat[edge['table']] = 1 + materials.index('table')
  mat[edge['furnace']] = 1 + materials.index('furnace')
  for item, amount in scenarios.RICH.items():
    inv[items.index(item)] = amount
