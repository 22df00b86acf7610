"""The C-ABI library loads on a CPU-only host and exports every entry point include/fsv2v.h declares; the Python binding
is derived from that header and agrees with it signature by signature."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, 'include', 'fsv2v.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\bint\s+(fsv_[a-z0-9_]+)\s*\(', text)))


def test_header_declares_entry_points():
    syms = declared_symbols()
    assert len(syms) >= 20 and 'fsv_conv_gather_fwd' in syms and 'fsv_warp_fwd' in syms


def test_no_setter_style_entry_points():
    """The header promises a library without state between calls (the resample2d_cuda.cc:6-31 convention): no entry point
    "arms" a later call - workspaces and side outputs are explicit, nullable arguments of the call that uses them.  Every
    declared function returns an int status (a `void` or pointer-returning function would be a setter / getter), none is
    named like one, and no kernel source keeps thread-local hand-over slots (the per-thread launch STATUS is the one
    thread_local the sources may hold: it is written and consumed inside one call)."""
    text = open(os.path.join(ROOT, 'include', 'fsv2v.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    non_int = re.findall(r'^\s*(?:void|float|double|long long|const \w+|\w+)\s*\*?\s+\*?(fsv_[a-z0-9_]+)\s*\(', text, flags=re.M)
    non_int = [n for n in non_int if n not in declared_symbols()]
    assert not non_int, non_int
    bad = [s for s in declared_symbols() if re.search(r'_(set|arm|armed|taken)$', s) or re.search(r'_(set|arm)_', s)]
    assert not bad, bad
    csrc = os.path.join(ROOT, 'few-shot-vid2vid_amd', 'csrc')
    for name in sorted(os.listdir(csrc)):
        src = open(os.path.join(csrc, name)).read()
        for m in re.finditer(r'thread_local\s+[^;=]+', src):
            assert 'fsv_launch_status' in m.group(0), (name, m.group(0))


@pytest.mark.parametrize('libname', ['libfsv2v_hip.so'])
def test_library_exports_every_declared_symbol(libname):
    import importlib
    import fsv2v_amd  # noqa: F401
    build = importlib.import_module('few-shot-vid2vid_amd.build')
    path = build.build_hip()           # hipcc cross-compiles for gfx950 without a GPU
    handle = ctypes.CDLL(path)
    missing = [s for s in declared_symbols() if not hasattr(handle, s)]
    assert not missing, missing


def _lib():
    import importlib
    import fsv2v_amd  # noqa: F401
    return importlib.import_module('few-shot-vid2vid_amd.lib')


def test_python_binding_table_matches_header():
    """the binding is derived from the header: it names exactly the declared entry points, each once"""
    import importlib
    lib = _lib()
    importlib.import_module('few-shot-vid2vid_amd.ops')
    importlib.import_module('few-shot-vid2vid_amd.profile')
    assert set(lib._SIGS) == set(declared_symbols())
    assert len(lib._SIGS) == len(declared_symbols())


def test_derived_argtypes_match_hand_written_expectations():
    """one declaration per type the mapping knows, written out by hand from include/fsv2v.h"""
    p, i, ll, f, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_float, ctypes.c_double
    sigs = _lib()._SIGS
    assert sigs['fsv_act_fwd'] == [p, p, ll, i, p]
    assert sigs['fsv_norm_stats_from_sums'] == [p, d, p, p, i, f, p, p, f, p]
    assert sigs['fsv_stamp_rate_khz'] == []
    assert sigs['fsv_spade_mod_bwd_h'] == ([p, p, p, p, i] + [p] * 10 + [i, i, i, i, ll, i, i, i, i, p, p, i, ll, p])
    assert len(sigs['fsv_spade_mod_bwd_h']) == 29
    assert sigs['fsv_prep_weight_grouped'] == [p, p, p, p, p, i, p]          # `const unsigned long long* taps` is a pointer
    assert sigs['fsv_stamp'] == [p, p]
    assert sigs['fsv_conv_gather_group'] == [p, i, i, p]                     # descriptor pointer
    assert sigs['fsv_hconv_gather'] == [p, i, p, p]
    assert sigs['fsv_spade_prep_h'] == [p, p, ll, ll, p, i, i, i, p]


@pytest.mark.parametrize('decl', ['int fsv_x(unsigned n);', 'int fsv_x(size_t n);', 'int fsv_x(int);', 'float fsv_x(int n);',
                                  'int fsv_x(int n); int fsv_x(int n);', 'int fsv_x(int (*cb)(int));',
                                  'typedef struct fsv_d { short a; } fsv_d;', 'typedef struct fsv_d { float *a, b; } fsv_d;'])
def test_parser_refuses_what_it_does_not_know(tmp_path, decl):
    lib = _lib()
    path = tmp_path / 'h.h'
    path.write_text(decl + '\n')
    with pytest.raises(lib.FsvError):
        lib.parse_header(str(path))


def test_parser_scalars_by_value(tmp_path):
    lib = _lib()
    path = tmp_path / 'h.h'
    path.write_text('int fsv_x(unsigned long long a, long long b, double c, float d, const int e, fsv_stream_t s, /* int z, */\n'
                    '          float* const* q);\n')
    sigs, structs, enums = lib.parse_header(str(path))
    assert sigs == {'fsv_x': [ctypes.c_ulonglong, ctypes.c_longlong, ctypes.c_double, ctypes.c_float, ctypes.c_int,
                              ctypes.c_void_p, ctypes.c_void_p]}


def _call_sites():
    """(file, line, [entry point names], number of positional arguments or None when the call unpacks *args) of every
    lib.call / lib.call_status in the package; names is None where the name is not a literal"""
    import ast
    pkg = os.path.join(ROOT, 'few-shot-vid2vid_amd')
    for fn in sorted(os.listdir(pkg)):
        if not fn.endswith('.py'):
            continue
        for node in ast.walk(ast.parse(open(os.path.join(pkg, fn)).read())):
            if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in ('call', 'call_status')
                    and isinstance(node.func.value, ast.Name) and node.func.value.id == 'lib' and node.args):
                continue
            first = node.args[0]
            alts = [first.body, first.orelse] if isinstance(first, ast.IfExp) else [first]
            names = [a.value for a in alts if isinstance(a, ast.Constant) and isinstance(a.value, str)]
            nargs = None if any(isinstance(a, ast.Starred) for a in node.args) or node.keywords else len(node.args) - 1
            yield fn, node.lineno, names if len(names) == len(alts) else None, nargs


def test_every_call_site_passes_the_declared_number_of_arguments():
    """ctypes takes surplus arguments of a cdecl function silently, so the count is checked here, statically: every call with a
    literal entry point name names a declared function and passes exactly its parameters"""
    sigs = _lib()._SIGS
    checked, unpacked, by_variable, wrong = 0, [], [], []
    for fn, line, names, nargs in _call_sites():
        if names is None:
            by_variable.append((fn, line))
        elif any(n not in sigs for n in names):
            wrong.append((fn, line, names, 'not declared'))
        elif nargs is None:
            unpacked.append((fn, line))
        else:
            checked += 1
            wrong += [(fn, line, n, nargs, len(sigs[n])) for n in names if len(sigs[n]) != nargs]
    assert not wrong, wrong
    # 108 sites are checked today; 5 unpack a prepared argument tuple (`*args`), 6 take the name from a variable (the launch
    # groups and profiler replays of conv.py, which re-issue one of those 5): the unchecked share must stay this small
    assert checked >= 100, checked
    assert len(unpacked) <= 5, unpacked
    assert len(by_variable) <= 6, by_variable


def test_descriptor_struct_layouts():
    """size and every field offset of the classes generated from the header's typedefs = those of the hand-written
    ctypes.Structure classes they replaced (the numbers were read off those classes)"""
    import importlib
    _lib()
    conv = importlib.import_module('few-shot-vid2vid_amd.conv')
    hconv = importlib.import_module('few-shot-vid2vid_amd.hconv')
    want = {
        conv.ConvDesc: (280, {'inp': 0, 'wt': 8, 'bias': 16, 'res': 24, 'out': 32, 'wscale': 40, 'N': 48, 'H': 52, 'W': 56,
                              'Cin': 60, 'OH': 64, 'OW': 68, 'Cout': 72, 'ntaps': 76, 'ty': 80, 'tx': 144, 'sy': 208, 'sx': 212,
                              'outH': 216, 'outW': 220, 'osy': 224, 'osx': 228, 'ooy': 232, 'oox': 236, 'ldw': 240,
                              'per_sample': 244, 'act': 248, 'accumulate': 252, 'scale': 256, 'w_bstride': 264,
                              'b_bstride': 272}),
        conv.WgradDesc: (216, {'inp': 0, 'dout': 8, 'dwt': 16, 'N': 24, 'H': 28, 'W': 32, 'Cin': 36, 'OH': 40, 'OW': 44,
                               'Cout': 48, 'ntaps': 52, 'ty': 56, 'tx': 120, 'sy': 184, 'sx': 188, 'ldw': 192, 'Kpad': 196,
                               'per_sample': 200, 'reserved': 204, 'w_bstride': 208}),
        hconv.HConvDesc: (328, {'inp': 0, 'wt': 8, 'bias': 16, 'res': 24, 'out': 32, 'wscale': 40, 'ws': 48, 'stats': 56,
                                'N': 64, 'H': 68, 'W': 72, 'Cin': 76, 'OH': 80, 'OW': 84, 'Cout': 88, 'ntaps': 92, 'ty': 96,
                                'tx': 160, 'sy': 224, 'sx': 228, 'outH': 232, 'outW': 236, 'osy': 240, 'osx': 244, 'ooy': 248,
                                'oox': 252, 'Kpad': 256, 'nrows': 260, 'per_sample': 264, 'act': 268, 'accumulate': 272,
                                'out_h': 276, 'res_h': 280, 'force_tile': 284, 'force_split': 288, 'stats_groups': 292,
                                'stats_slots': 296, 'stats_prezeroed': 300, 'scale': 304, 'w_bstride': 312, 'b_bstride': 320}),
    }
    assert [c.__name__ for c in want] == ['ConvDesc', 'WgradDesc', 'HConvDesc']
    for cls, (size, offsets) in want.items():
        assert ctypes.sizeof(cls) == size
        assert [name for name, _ in cls._fields_] == list(offsets)
        assert {name: getattr(cls, name).offset for name in offsets} == offsets
        assert cls.ty.size == cls.tx.size == 64


def test_activation_codes_come_from_the_header():
    import importlib
    lib = _lib()
    conv = importlib.import_module('few-shot-vid2vid_amd.conv')
    assert (conv.ACT_NONE, conv.ACT_LRELU, conv.ACT_TANH, conv.ACT_SIGMOID, conv.ACT_RELU, conv.ACT_LRELU01,
            conv.ACT_DLRELU) == (0, 1, 2, 3, 4, 5, 6)
    assert lib.ENUMS['FSV_OK'] == 0 and lib.ENUMS['FSV_ERR_UNSUPPORTED'] == -2


def test_product_path_refuses_to_run_without_the_hip_library(monkeypatch, tmp_path):
    """No silent fallback: with the emulation switch off and no libfsv2v_hip.so the loader raises."""
    import importlib
    import fsv2v_amd  # noqa: F401
    lib = importlib.import_module('few-shot-vid2vid_amd.lib')
    monkeypatch.setenv('FSV2V_EMU', '0')
    monkeypatch.setattr(lib, '_lib', None)
    monkeypatch.setattr(lib, '_is_emu', lib._is_emu)      # get_lib() rewrites it: have it restored afterwards
    monkeypatch.setattr(lib, '_HERE', str(tmp_path))
    with pytest.raises(lib.FsvError):
        lib.get_lib()
    monkeypatch.setattr(lib, '_lib', None)


def test_host_tensors_are_rejected_by_the_hip_binding(monkeypatch):
    import importlib
    import torch
    import fsv2v_amd  # noqa: F401
    lib = importlib.import_module('few-shot-vid2vid_amd.lib')
    monkeypatch.setattr(lib, '_is_emu', False)
    monkeypatch.setattr(lib, '_lib', object())
    with pytest.raises(lib.FsvError):
        lib.check_device(torch.zeros(4))
    monkeypatch.setattr(lib, '_lib', None)
