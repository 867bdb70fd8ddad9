"""Authored worlds: a bank of caller-designed worlds that `BatchedEnv.reset(worlds=bank)` resets envs into
(include/crafter_hip.h crafter_reset_worlds).  This module is the host side -- building, checking, saving a bank -- and needs no
device until the bank is uploaded."""
import numpy as np

from . import abi, tables

CLASS_NAMES = ('player', 'cow', 'zombie', 'skeleton', 'arrow', 'plant')   # CRAFTER_T_* 1 .. 6
CLASS_IDS = {n: i + 1 for i, n in enumerate(CLASS_NAMES)}
# health a fresh object of the class has (objects.py:266, 285, 318, 391; the player's lives in the inventory, an arrow has none)
CLASS_HEALTH = {abi.T_PLAYER: 0, abi.T_COW: 3, abi.T_ZOMBIE: 5, abi.T_SKELETON: 3, abi.T_ARROW: 0, abi.T_PLANT: 1}
FACING_CLASSES = (abi.T_PLAYER, abi.T_ARROW)   # the classes that keep a facing; the others' is stored as (0, 0)


def _geometry(batch_or_geometry):
  """-> (W, H, rules dict) of a BatchedEnv / anything with .cfg and .rules (or .rules_dict), or of dict(area=..., rules=...)."""
  g = batch_or_geometry
  if isinstance(g, dict):
    area = g.get('area', (64, 64))
    return int(area[0]), int(area[1]), g.get('rules') or tables.load_rules()
  rules = getattr(g, 'rules', None) or getattr(g, 'rules_dict', None) or tables.load_rules()
  return int(g.cfg.W), int(g.cfg.H), rules


def _record(obj):
  """One object as given -- a dict or a tuple (type, x, y, health=class default, facing=(0, 1), aux=0) -> the six values."""
  if isinstance(obj, dict):
    unknown = set(obj) - {'type', 'x', 'y', 'health', 'facing', 'aux'}
    if unknown:
      raise ValueError(f'unknown object fields {sorted(unknown)}')
    typ, x, y = obj['type'], obj['x'], obj['y']
    health, facing, aux = obj.get('health'), obj.get('facing', (0, 1)), obj.get('aux', 0)
  else:
    obj = tuple(obj)
    if not 3 <= len(obj) <= 6:
      raise ValueError(f'an object is (type, x, y[, health[, facing[, aux]]]), got {obj!r}')
    typ, x, y = obj[:3]
    health = obj[3] if len(obj) > 3 else None
    facing = obj[4] if len(obj) > 4 else (0, 1)
    aux = obj[5] if len(obj) > 5 else 0
  if isinstance(typ, str):
    if typ.lower() not in CLASS_IDS:
      raise ValueError(f'unknown object class {typ!r} (one of {CLASS_NAMES})')
    typ = CLASS_IDS[typ.lower()]
  typ = int(typ)
  if health is None:
    health = CLASS_HEALTH.get(typ, 0)
  fx, fy = facing
  return typ, int(x), int(y), int(health), int(fx), int(fy), int(aux)


def worlds_of(mat, objs, rec, n_items):
  """State rows read back from a batch -- mat [K, W, H], objs (structured [K, C]), rec (structured [K]) -> the worlds they hold, in
  the form WorldBank accepts: dict(mat, objects: the live objects in slot order, the player first, inventory [K, n_items])."""
  objects = []
  for j in range(len(rec)):
    row = []
    for s in range(1, int(rec[j]['nobj'])):
      o = objs[j, s]
      if o['type'] == abi.T_NONE:
        continue
      health = 0 if o['type'] == abi.T_PLAYER else int(o['health'])
      row.append((int(o['type']), int(o['x']), int(o['y']), health, (int(o['fx']), int(o['fy'])), int(o['aux'])))
    objects.append(row)
  return dict(mat=np.array(mat, np.uint8), objects=objects, inventory=np.array(rec['inv'][:, :n_items], np.int32))


class WorldBank:
  """K authored worlds of one geometry.
  mat: [K, W, H] material ids (1 .. n_materials) or material names, indexed [x][y] as the reference's world map.
  objects: per world a list of dicts / tuples (type, x, y, health=class default, facing=(0, 1), aux=0), class names accepted;
    applied in order through World.add, so slots are 2, 3, ... in list order.  A 'player' entry is allowed as the FIRST one only:
    it moves the player (who is otherwise added at the centre) and sets the facing.  aux is the zombie's cooldown, the
    skeleton's reload, the plant's `grown`.
  inventory: None (the rules' initial inventory) or [K, n_items] / per world a dict of item names.
  Everything the device would flag (CRAFTER_ST_BAD_WORLD) raises ValueError here; validate=False skips those checks and
  leaves them to the device."""

  def __init__(self, batch_or_geometry, mat, objects, inventory=None, validate=True):
    W, H, rules = _geometry(batch_or_geometry)
    self.area = (W, H)
    self.material_names = list(rules['materials'])
    self.item_names = list(rules['items'])
    item_max = [int(rules['items'][n]['max']) for n in self.item_names]
    item_init = [int(rules['items'][n]['initial']) for n in self.item_names]
    nmat = len(self.material_names)
    m = np.asarray(mat)
    if m.dtype.kind in 'USO':
      ids = {n: i + 1 for i, n in enumerate(self.material_names)}
      try:
        m = np.vectorize(lambda s: ids[str(s)], otypes=[np.int64])(m)
      except KeyError as e:
        raise ValueError(f'unknown material {e.args[0]!r}') from None
    if m.ndim == 2:
      m = m[None]
    if m.ndim != 3 or m.shape[1:] != (W, H):
      raise ValueError(f'mat must be [K, {W}, {H}], got {m.shape}')
    if m.dtype.kind not in 'iu':
      raise ValueError('mat must hold material ids or names')
    if validate and (m.min() < 1 or m.max() > nmat):
      raise ValueError(f'material ids must lie in 1 .. {nmat}')
    if m.min() < 0 or m.max() > 255:
      raise ValueError('material ids must fit a byte')
    K = m.shape[0]
    self.mat = np.ascontiguousarray(m.astype(np.uint8))
    objects = list(objects)
    if len(objects) != K:
      raise ValueError(f'{K} maps, {len(objects)} object lists')
    recs = [[_record(o) for o in world] for world in objects]
    cap = max([len(r) for r in recs] + [1])
    self.objs = np.zeros((K, cap), abi.OBJ_DTYPE)
    self.nobj = np.array([len(r) for r in recs], np.int32)
    for j, world in enumerate(recs):
      taken = {(W // 2, H // 2)}
      for k, (typ, x, y, health, fx, fy, aux) in enumerate(world):
        where = f'world {j} object {k}'
        if validate:
          if not abi.T_PLAYER <= typ <= abi.T_PLANT:
            raise ValueError(f'{where}: class id {typ} is none of 1 .. 6')
          if not (0 <= x < W and 0 <= y < H):
            raise ValueError(f'{where}: cell ({x}, {y}) lies outside the {W} x {H} world')
          if typ == abi.T_PLAYER and k != 0:
            raise ValueError(f'{where}: the player may only be the first object of a world')
          if typ in FACING_CLASSES and fx * fx + fy * fy != 1:
            raise ValueError(f'{where}: facing ({fx}, {fy}) is no unit axis vector')
          if typ == abi.T_PLAYER:
            taken = {(x, y)}
          elif (x, y) in taken:
            raise ValueError(f'{where}: cell ({x}, {y}) is already occupied')
          taken.add((x, y))
        if not (0 <= typ <= 255 and 0 <= x <= 65535 and 0 <= y <= 65535 and -128 <= health <= 127 and -128 <= fx <= 127 and
                -128 <= fy <= 127 and -2 ** 31 <= aux < 2 ** 31):
          raise ValueError(f'{where}: a value does not fit its field of the object record')
        self.objs[j, k] = (typ, health, fx, fy, x, y, aux, 0)
    if inventory is None:
      self.inv = None
    else:
      rows = []
      for j, row in enumerate(inventory):
        if isinstance(row, dict):
          unknown = set(row) - set(self.item_names)
          if unknown:
            raise ValueError(f'world {j}: unknown items {sorted(unknown)}')
          row = [row.get(n, item_init[i]) for i, n in enumerate(self.item_names)]
        row = [int(v) for v in row]
        if len(row) != len(self.item_names):
          raise ValueError(f'world {j}: the inventory has {len(row)} entries, the rules {len(self.item_names)} items')
        if any(v < 0 or v > hi for v, hi in zip(row, item_max)):
          raise ValueError(f'world {j}: an inventory value lies outside 0 .. the item\'s maximum')
        rows.append(row)
      if len(rows) != K:
        raise ValueError(f'{K} maps, {len(rows)} inventories')
      self.inv = np.array(rows, np.int32).reshape(K, len(self.item_names))
    self._device = {}

  def __len__(self):
    return int(self.mat.shape[0])

  @property
  def max_objects(self):
    """Slots the longest world needs: slot 0, the player, its objects."""
    return 2 + int(self.nobj.max(initial=0))

  def worlds(self):
    """-> dict(mat, objects, inventory) in the form the constructor accepts (what BatchedEnv.export_worlds returns)."""
    objects = [[(int(o['type']), int(o['x']), int(o['y']), int(o['health']), (int(o['fx']), int(o['fy'])), int(o['aux']))
                for o in self.objs[j, :self.nobj[j]]] for j in range(len(self))]
    return dict(mat=self.mat.copy(), objects=objects, inventory=None if self.inv is None else self.inv.copy())

  def device_tensors(self, device):
    """The bank as device tensors (uploaded once per device): mat, objs (bytes), nobj, inv or None."""
    import torch
    key = str(device)
    if key not in self._device:
      up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
      self._device[key] = dict(mat=up(self.mat.reshape(len(self), -1)), objs=up(self.objs.view(np.uint8).reshape(len(self), -1)),
                               nobj=up(self.nobj), inv=None if self.inv is None else up(self.inv))
    return self._device[key]

  def save(self, path):
    """One .npz that WorldBank.load reads back (python -m crafter_amd.run_random --worlds FILE.npz plays it)."""
    np.savez_compressed(path, area=np.array(self.area, np.int32), mat=self.mat, objs=self.objs.view(np.uint8).reshape(len(self), -1),
                        nobj=self.nobj, inv=np.zeros((0, 0), np.int32) if self.inv is None else self.inv)

  @classmethod
  def load(cls, path, rules=None):
    g = np.load(path)
    objs = np.ascontiguousarray(g['objs']).view(abi.OBJ_DTYPE).reshape(len(g['nobj']), -1)
    objects = [[(int(o['type']), int(o['x']), int(o['y']), int(o['health']), (int(o['fx']), int(o['fy'])), int(o['aux']))
                for o in objs[j, :g['nobj'][j]]] for j in range(len(g['nobj']))]
    inv = g['inv'] if g['inv'].size else None
    return cls(dict(area=tuple(int(v) for v in g['area']), rules=rules), g['mat'], objects, inv)
