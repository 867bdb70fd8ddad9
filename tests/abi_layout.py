"""TEST INFRASTRUCTURE: what include/crafter_hip_types.h (and crafter_hip.h's crafter_host_tables) say, as a C compiler reads
them, next to what crafter_amd/abi.py and lib.HostTablesC say.  A C99 program is generated from the Python side's own field
lists, compiled against the headers alone and run once per session."""
import ctypes as C
import functools
import pathlib
import re
import subprocess
import tempfile

ROOT = pathlib.Path(__file__).resolve().parent.parent
INCLUDE = ROOT / 'include'
VALUE_NAME = r'(?:T|A|ST|TEX|MAX)_[A-Z0-9_]+|MT_N|CHUNK'


def python_layouts():
  """C struct name -> (sizeof, [(field, offset, size, is_aggregate)]) as the ctypes classes and numpy dtypes lay them out."""
  from crafter_amd import abi, lib

  def ct(cls):
    return C.sizeof(cls), [(name, getattr(cls, name).offset, getattr(cls, name).size, issubclass(tp, (C.Array, C.Structure)))
                           for name, tp in cls._fields_]

  def npy(dt):
    return dt.itemsize, [(name, dt.fields[name][1], dt.fields[name][0].itemsize, bool(dt.fields[name][0].shape)) for name in dt.names]

  return {
      'crafter_obj': npy(abi.OBJ_DTYPE), 'crafter_item_list': ct(abi.ItemList), 'crafter_collect_rule': ct(abi.CollectRule),
      'crafter_place_rule': ct(abi.PlaceRule), 'crafter_make_rule': ct(abi.MakeRule), 'crafter_rules': ct(abi.Rules),
      'crafter_config': ct(abi.Config), 'crafter_env_rec': npy(abi.REC_DTYPE), 'crafter_pool_hdr': npy(abi.POOL_HDR_DTYPE),
      'crafter_state_ptrs': ct(abi.StatePtrs), 'crafter_host_tables': ct(lib.HostTablesC),
  }


def python_values():
  """abi.py's constants and enum values by their short names (T_*, A_*, ST_*, TEX_*, MAX_*, MT_N, CHUNK)."""
  from crafter_amd import abi
  return {name: value for name, value in vars(abi).items() if re.fullmatch(VALUE_NAME, name)}


def header_value_names():
  """The short names of every CRAFTER_<T|A|ST|TEX|MAX>_* / CRAFTER_MT_N / CRAFTER_CHUNK the header spells (a word search: the
  values come from the compiler)."""
  return set(re.findall(rf'\bCRAFTER_({VALUE_NAME})\b', (INCLUDE / 'crafter_hip_types.h').read_text()))


def program(layouts, value_names):
  """The C99 text.  One positional initializer per Python field (0, or {0} for an array / struct): with -Wextra -Werror a
  field the Python side lacks is a 'missing initializer' error and one it has too many an 'excess elements' error, so the
  field COUNT of each struct is the compiler's, padding or not ({0} opens an array of structs too: -Wno-missing-braces)."""
  out = ['#include <stdio.h>', '#include "crafter_hip.h"', '']
  for struct, (_, fields) in layouts.items():
    out.append(f'static const {struct} count_{struct} = {{ {", ".join("{0}" if agg else "0" for *_, agg in fields)} }};')
  out += ['', 'int main(void) {']
  for struct, (_, fields) in layouts.items():
    out.append(f'  printf("S {struct} %lu\\n", (unsigned long)sizeof({struct}));')
    out.append(f'  (void)count_{struct};')
    for name, *_ in fields:
      out.append(f'  printf("F {struct} {name} %lu %lu\\n", (unsigned long)offsetof({struct}, {name}), '
                 f'(unsigned long)sizeof((({struct}*)0)->{name}));')
  for name in sorted(value_names):
    out.append(f'  printf("V {name} %ld\\n", (long)CRAFTER_{name});')
  out += ['  return 0;', '}', '']
  return '\n'.join(out)


@functools.lru_cache(maxsize=None)
def header_report():
  """-> ({struct: sizeof}, {(struct, field): (offset, size)}, {short name: value}) as gcc -std=c99 -pedantic reads the headers."""
  names = header_value_names() | set(python_values())
  with tempfile.TemporaryDirectory() as tmp:
    src, exe = pathlib.Path(tmp) / 'abi_layout.c', pathlib.Path(tmp) / 'abi_layout'
    src.write_text(program(python_layouts(), names))
    cmd = ['gcc', '-std=c99', '-Wall', '-Wextra', '-Werror', '-Wno-missing-braces', '-pedantic', f'-I{INCLUDE}', str(src), '-o', str(exe)]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr
    text = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
  sizes, fields, values = {}, {}, {}
  for line in text.splitlines():
    kind, *rest = line.split()
    if kind == 'S':
      sizes[rest[0]] = int(rest[1])
    elif kind == 'F':
      fields[rest[0], rest[1]] = (int(rest[2]), int(rest[3]))
    else:
      values[rest[0]] = int(rest[1])
  return sizes, fields, values
