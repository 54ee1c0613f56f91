"""The whole C boundary in one place: include/whmr_hip.h against whmr_amd/_lib.py.  Entry-point names, the set of structs, every struct's layout
as gcc sees it, the ``struct`` formats the host packs device tables with, and the argument types of every prototype.  All of it is driven by the
header and by ``_lib.C_STRUCTS`` / ``_lib._SIGS``: a new entry point or struct needs no new test code, and one left out on either side fails here."""
import ctypes as C
import os
import re
import struct
import subprocess

import pytest

from conftest import ROOT
from whmr_amd import _lib as L
from whmr_amd.train import optim

# the structs whose rows the host packs, each with the format the package REALLY packs it with
PACKED = {'whmr_augment_item': L.AUGMENT_ITEM_FORMAT, 'whmr_frame_crop_item': L.FRAME_CROP_ITEM_FORMAT, 'whmr_wprep_item': L._WPREP_ITEM.format,
          'whmr_adam_item': optim._ITEM.format, 'whmr_adam_hyper': optim._HYPER.format, 'whmr_adam_guard_cfg': optim._GUARD_CFG.format,
          'whmr_adam_guard_state': optim._GUARD_STATE.format}
PINNED_SIZES = {'whmr_augment_item': 304, 'whmr_frame_crop_item': 72, 'whmr_adam_guard_cfg': 16, 'whmr_adam_guard_state': 32}
CONSTANTS = {'WHMR_ADAM_CHUNK': L.ADAM_CHUNK, 'WHMR_LOSS_STAGES': L.LOSS_STAGES, 'WHMR_LOSS_TERMS': L.LOSS_TERMS}


def _header():
    """the header without its comments (one prototype has a comment inside its parameter list)"""
    text = open(os.path.join(ROOT, 'include', 'whmr_hip.h')).read()
    return re.sub(r'//[^\n]*', ' ', re.sub(r'/\*.*?\*/', ' ', text, flags=re.S))


def _header_structs():
    """{struct name: its field names in order}; 'const double *pose, *betas; double T[9], M[6];' -> pose, betas, T, M"""
    out = {}
    for name, body in re.findall(r'\bstruct\s+(whmr_\w+)\s*\{([^}]*)\}', _header()):
        pieces = [p for decl in body.split(';') for p in decl.split(',') if p.strip()]
        out[name] = [re.search(r'(\w+)\s*(?:\[[^\]]*\])?\s*$', p).group(1) for p in pieces]
    return out


def _mirrors():
    return [v for v in vars(L).values() if isinstance(v, type) and issubclass(v, C.Structure) and v.__module__ == L.__name__]


def test_library_builds_and_exports_every_declared_symbol():
    import __graft_entry__ as ge
    ge.build()
    lib = C.CDLL(L.LIB_PATH)
    declared = set(re.findall(r'^\s*int\s+(whmr_\w+)\s*\(', _header(), flags=re.M))
    assert declared and declared == set(L.EXPORTS)
    for name in declared:
        assert getattr(lib, name) is not None


def test_every_struct_of_the_header_has_one_registered_mirror():
    assert set(_header_structs()) == set(L.C_STRUCTS) and len(L.C_STRUCTS) == len(set(L.C_STRUCTS.values()))
    unregistered = [m.__name__ for m in _mirrors() if m not in L.C_STRUCTS.values()]
    assert not unregistered, unregistered


def test_mirrors_and_constants_match_the_c_header_layout(tmp_path):
    """the drop-in boundary is a C ABI: every ctypes mirror has the field names of its struct in include/whmr_hip.h, in the header's order, and the
    size and field offsets gcc gives it (a field added on one side only, or a wrong width, would shift every pointer behind it); the #defines the
    package restates have the header's values"""
    structs = _header_structs()
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "whmr_hip.h"', 'int main(void) {']
    lines += ['  printf("%s %%d\\n", %s);' % (k, k) for k in CONSTANTS]
    for cname, fields in structs.items():
        lines.append('  printf("%s %%zu\\n", sizeof(struct %s));' % (cname, cname))
        lines += ['  printf("%s.%s %%zu\\n", offsetof(struct %s, %s));' % (cname, f, cname, f) for f in fields]
    lines += ['  return 0;', '}']
    src, exe = tmp_path / 'layout.c', tmp_path / 'layout'
    src.write_text('\n'.join(lines))
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    got = {k: int(v) for k, v in (l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())}
    assert {k: got[k] for k in CONSTANTS} == CONSTANTS
    assert len(structs) == 17
    for cname, fields in structs.items():
        cls = L.C_STRUCTS[cname]
        assert [f for f, _ in cls._fields_] == fields, cname
        assert got[cname] == C.sizeof(cls), (cname, got[cname], C.sizeof(cls))
        for f in fields:
            assert got['%s.%s' % (cname, f)] == getattr(cls, f).offset, (cname, f)
    assert [f for f, _ in L._WhmrLossStage._fields_][:L.LOSS_TERMS] == list(L.LOSS_FIELDS)     # field k belongs to term k


@pytest.mark.parametrize('cname', PACKED)
def test_packed_row_format_puts_every_value_in_its_field(cname):
    """the format a table's rows are packed with is the one derived from the mirror, has the mirror's size, and a row of distinct values read back
    through the mirror has each value in the field it was meant for"""
    cls, fmt = L.C_STRUCTS[cname], PACKED[cname]
    assert fmt == L.struct_format(cls)
    assert struct.calcsize(fmt) == C.sizeof(cls) == PINNED_SIZES.get(cname, C.sizeof(cls))
    want, k = {}, 0
    for name, t in cls._fields_:
        n, t = (t._length_, t._type_) if issubclass(t, C.Array) else (1, t)
        vals = [(k + i + 1.5) if t in (C.c_float, C.c_double) else 0x101 * (k + i + 1) for i in range(n)]       # k + 1.5: exact in fp32
        want[name], k = (vals if n > 1 else vals[0]), k + n
    row = cls.from_buffer_copy(struct.pack(fmt, *[v for vs in want.values() for v in (vs if isinstance(vs, list) else [vs])]))
    assert {name: (list(getattr(row, name)) if isinstance(v, list) else getattr(row, name)) for name, v in want.items()} == want


def test_packed_rows_of_known_values():
    it = L._WhmrFrameCropItem.from_buffer_copy(struct.pack(L.FRAME_CROP_ITEM_FORMAT, 0x1234, 7, 9, 27, *range(6)))
    assert (it.frame, it.H, it.W, it.row_stride, list(it.inv)) == (0x1234, 7, 9, 27, [0.0, 1.0, 2.0, 3.0, 4.0, 5.0])
    hyper = L._WhmrAdamHyper.from_buffer_copy(optim._HYPER.pack(0.9, 0.999, 5e-5, 0.5, 0.125))
    assert (hyper.beta1, hyper.beta2, hyper.lr, hyper.eps, hyper.weight_decay) == (0.9, 0.999, 5e-5, 0.5, 0.125)       # betas and lr: doubles, kept exactly
    cfg = L._WhmrAdamGuardCfg.from_buffer_copy(optim._GUARD_CFG.pack(0.75, 1, 0))
    assert (cfg.max_norm, cfg.skip_nonfinite) == (0.75, 1)
    state = L._WhmrAdamGuardState.from_buffer_copy(optim._GUARD_STATE.pack(1.5, 0.25, 1, 0, 7, 3))
    assert (state.grad_norm, state.clip_coef, state.apply, state.steps_seen, state.steps_skipped) == (1.5, 0.25, 1, 7, 3)


_INT64 = (C.c_long, C.c_longlong, C.c_int64)
_BY_VALUE = {'int': (C.c_int,), 'int32_t': (C.c_int,), 'float': (C.c_float,), 'double': (C.c_double,), 'long': _INT64, 'int64_t': _INT64,
             'long long': _INT64}
_POINTEES = {'void': None, 'float': C.c_float, 'double': C.c_double, 'int': C.c_int, 'long': C.c_long, 'unsigned': C.c_uint,
             'unsigned long long': C.c_ulonglong}
_POINTEES.update({'%sint%d_t' % (u, n): getattr(C, 'c_%sint%d' % (u, n)) for u in ('', 'u') for n in (8, 16, 32, 64)})


def _accepted(param):
    """the ctypes argument types that pass one C parameter correctly; an unknown C type raises"""
    m = re.fullmatch(r'(struct\s+)?([\w ]+?)\s*(\**)\s*\w+', re.sub(r'\bconst\b', ' ', param).strip())
    is_struct, base, stars = m.group(1), ' '.join(m.group(2).split()), m.group(3)
    if not stars:
        return _BY_VALUE[base]
    if is_struct:                                    # c_void_p: Python passes a packed array of them
        return (C.POINTER(L.C_STRUCTS[base]), C.c_void_p)
    return (C.c_void_p,) + ((C.POINTER(_POINTEES[base]),) if _POINTEES[base] else ())


def test_argument_types_of_every_prototype_match_the_header():
    """_SIGS against the header, parameter by parameter: an int typed where the header says long (a stride, an element count) truncates silently"""
    assert C.sizeof(C.c_int) == 4 and all(C.sizeof(t) == 8 for t in _INT64)
    protos = dict(re.findall(r'\bint\s+(whmr_\w+)\s*\(([^)]*)\)\s*;', _header()))
    assert set(protos) == set(L._SIGS)
    for name, params in protos.items():
        params = [p.strip() for p in params.split(',')]
        assert len(params) == len(L._SIGS[name]), (name, len(params), len(L._SIGS[name]))
        for i, (param, got) in enumerate(zip(params, L._SIGS[name])):
            try:
                accepted = _accepted(param)
            except (KeyError, AttributeError):
                pytest.fail('%s, parameter %d: no rule for the C type of "%s"' % (name, i, param))
            assert got in accepted, (name, i, param, got)
