"""ctypes binding of libcrafter_hip.so (include/crafter_hip.h).  There is no CPU path: if the
library is missing, cannot be loaded, or reports a different struct layout, import fails loudly."""
import ctypes as C
import pathlib

from . import abi

LIB_PATH = pathlib.Path(__file__).resolve().parent / '_lib' / 'libcrafter_hip.so'


class HostTablesC(C.Structure):
  _fields_ = [
      ('rules', C.c_void_p),
      ('atlas', C.c_void_p), ('atlas_bytes', C.c_size_t),
      ('tex_tile', C.c_void_p), ('n_tex_tile', C.c_int32),
      ('tex_icon', C.c_void_p), ('n_tex_icon', C.c_int32),
      ('tex_digit', C.c_void_p), ('n_tex_digit', C.c_int32),
      ('tex_alpha', C.c_void_p), ('n_tex_alpha', C.c_int32),
      ('item_pos', C.c_void_p), ('n_item_pos', C.c_int32),
      ('daylight', C.c_void_p), ('n_daylight', C.c_int32),
      ('vignette', C.c_void_p), ('n_vignette', C.c_int32),
      ('unit255', C.c_void_p), ('n_unit255', C.c_int32),
  ]


class CrafterLibError(RuntimeError):
  pass


vp, i32, i64, text = C.c_void_p, C.c_int32, C.c_int64, C.c_char_p
_state = C.POINTER(abi.StatePtrs)

# name -> (restype, argtypes, optional): one row per function include/crafter_hip.h declares, in the header's parameter
# order (tests/test_host_logic.py holds the table against the header, type class by type class).  optional: an A/B build of
# an older ABI, named by CRAFTER_HIP_LIB (tools/ab_make.sh), may lack the entry point -- everything else works.
SIGNATURES = {
    'crafter_struct_sizes': (None, [C.POINTER(i32)], False),
    'crafter_abi_version': (i32, [], False),
    'crafter_create': (i32, [C.POINTER(abi.Config), C.POINTER(vp)], False),
    'crafter_destroy': (None, [vp], False),
    'crafter_upload_tables': (i32, [vp, C.POINTER(HostTablesC)], False),
    'crafter_bind_state': (i32, [vp, _state], False),
    'crafter_lds_bytes': (i32, [vp], False),
    'crafter_slot_map_derived': (i32, [vp], False),
    'crafter_step_instance': (i32, [vp], False),
    'crafter_reset': (i32, [vp] * 4, False),
    'crafter_step': (i32, [vp] * 6, False),
    'crafter_step_n': (i32, [vp, i32] + [vp] * 5, False),
    'crafter_debug_dispatch_order': (i32, [vp, vp], False),
    'crafter_debug_set_dispatch_order': (i32, [vp, vp], False),
    'crafter_render': (i32, [vp] * 4, False),
    'crafter_set_timing': (i32, [vp, i32], False),
    'crafter_get_timing': (i32, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(i32)], False),
    'crafter_pool_status': (i32, [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)], False),
    'crafter_pool_error': (text, [vp], False),
    'crafter_last_error': (text, [vp], False),
    'crafter_debug_eval': (i32, [i32] + [vp] * 5 + [i64, vp], False),
    'crafter_extend_daylight': (i32, [vp, vp, i32], True),
    'crafter_exchange_unique_id': (i32, [vp], True),
    'crafter_exchange_create': (i32, [vp, i32, i32, i32, C.POINTER(vp)], True),
    'crafter_exchange_destroy': (None, [vp], True),
    'crafter_step_exchange': (i32, [vp, vp, i32, vp, vp, vp, i64, i64, i64, i32, vp], True),
    'crafter_exchange_wait': (i32, [vp, i32, vp], True),
    'crafter_exchange_error': (text, [vp], True),
    'crafter_copy_envs': (i32, [vp, vp, vp, i32] + [vp] * 4, True),
    'crafter_save_envs': (i32, [vp, vp, i32, vp, vp, vp, _state, i32, i32] + [vp] * 4, True),
    'crafter_load_envs': (i32, [vp, _state, i32, i32] + [vp] * 5 + [i32] + [vp] * 4, True),
    'crafter_symbolic': (i32, [vp] * 5, True),
    'crafter_step_final': (i32, [vp] * 10, True),
    'crafter_reseed': (i32, [vp] * 5, True),
    'crafter_legal_actions': (i32, [vp] * 4, True),
    'crafter_step_envs': (i32, [vp, vp, i32] + [vp] * 5, True),
    'crafter_set_levels': (i32, [vp] * 4 + [i32, C.c_uint64, vp], True),
    'crafter_level_ids': (i32, [vp] * 4, True),
    'crafter_reset_worlds': (i32, [vp] * 7 + [i32, i32, vp, vp], True),
    'crafter_step_n_envs': (i32, [vp, vp, i32, i32] + [vp] * 5, True),
}
EXPORTS = list(SIGNATURES)

# name -> (the header under include/ that declares it, restype, argtypes): entry points that extend the boundary from a header
# of their own, looked up by name.  Always optional: a library without one loads, and require() says what is missing.
EXTENSIONS = {
    'crafter_fingerprint': ('crafter_hip_fingerprint.h', i32, [vp, vp, C.c_uint32, vp, vp, vp]),
    'crafter_navigate': ('crafter_hip_navigate.h', i32, [vp, vp, vp, i32, C.c_uint32, vp, vp, vp, vp]),
    'crafter_edit_envs': ('crafter_hip_edit.h', i32, [vp, vp, i32, vp, i32, vp]),
    'crafter_audit': ('crafter_hip_audit.h', i32, [vp] * 5),
    'crafter_nearby': ('crafter_hip_nearby.h', i32, [vp, vp, i32, i32, C.c_uint32, i32, vp, vp, vp, vp]),
}

_lib = None


def load(path=None):
  """Loads (once) and type-annotates the shared library.  Raises CrafterLibError if it is absent:
  build it with ``python -m crafter_amd.build`` (hipcc, gfx950)."""
  global _lib
  if _lib is not None:
    return _lib
  import os
  older = bool(os.environ.get('CRAFTER_HIP_LIB'))   # env override: A/B builds, possibly of an older ABI
  path = pathlib.Path(path or os.environ.get('CRAFTER_HIP_LIB') or LIB_PATH)
  if not path.exists():
    raise CrafterLibError(
        f'{path} not found: the HIP extension is required (no CPU fallback). '
        'Build it with `python -m crafter_amd.build`.')
  try:
    lib = C.CDLL(str(path))
  except OSError as e:
    raise CrafterLibError(f'cannot load {path}: {e}') from e
  missing = []
  for name, (restype, argtypes, optional) in SIGNATURES.items():
    fn = getattr(lib, name, None)
    if fn is not None:
      fn.restype, fn.argtypes = restype, argtypes
    elif not (optional and older):
      missing.append(name)
  if missing:
    raise CrafterLibError(f'{path} lacks symbols {missing}')
  for name, (_, restype, argtypes) in EXTENSIONS.items():
    fn = getattr(lib, name, None)
    if fn is not None:
      fn.restype, fn.argtypes = restype, argtypes
  sizes = (i32 * 6)()
  lib.crafter_struct_sizes(sizes)
  abi.check_sizes(list(sizes))
  _lib = lib
  return lib


def require(lib, symbol, feature):
  """-> lib's entry point `symbol`; CrafterLibError if an older build (see `optional` above) lacks it."""
  fn = getattr(lib, symbol, None)
  if fn is None:
    raise CrafterLibError(f'the loaded library has no {symbol} (an older build): {feature} is not available')
  return fn


def last_error(lib, handle):
  msg = lib.crafter_last_error(handle)
  return msg.decode() if msg else 'unknown error'
