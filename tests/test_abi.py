"""CPU: dlsg_amd/abi.py reads include/dlsg.h as the C compiler does, and the library matches the header -- it loads, exports
every symbol the header declares, and every argument struct has the size and the member offsets the compilers gave it (no
compute calls: there is no GPU here)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from dlsg_amd import abi, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# dlsg_struct_size(i) is sizeof() of the i-th of these (csrc/attention.hip): the order the structs were added in, which the
# header cannot tell; dlsg_gemm_group, a member of dlsg_gemm_args, has no index
STRUCT_INDEX = ['dlsg_gemm_args', 'dlsg_rowln_args', 'dlsg_rowln_bwd_args', 'dlsg_o2v_args', 'dlsg_decatt_args', 'dlsg_decatt_bwd_args',
                'dlsg_lstm_pw_args', 'dlsg_lstm_pw_bwd_args', 'dlsg_dec_mid_args', 'dlsg_dec_tail_args', 'dlsg_dec_mid_bwd_args',
                'dlsg_decatt_cache_grads_args', 'dlsg_o2v_bwd_args', 'dlsg_latent_psl_args', 'dlsg_sa_core_args', 'dlsg_beam_select_args',
                'dlsg_gather_multi_args', 'dlsg_sa_core_bwd_args', 'dlsg_latent_psl_bwd_args', 'dlsg_bilstm_args', 'dlsg_bilstm_bwd_args',
                'dlsg_colsum_desc', 'dlsg_lstm_seq_args', 'dlsg_cln_args', 'dlsg_crit_sa_args', 'dlsg_crit_pattn_args', 'dlsg_crit_tsum_args',
                'dlsg_crit_score_args', 'dlsg_crit_colsum_desc', 'dlsg_crit_reduce_desc', 'dlsg_cider_tables']


def header_functions():
    txt = open(os.path.join(ROOT, 'include', 'dlsg.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(?:int|int64_t)\s+(dlsg_\w+)\s*\(', txt)))


def test_library_exports_every_declared_symbol():
    lib = hip.load_library()
    names = header_functions()
    assert len(names) >= 25
    for n in names:
        assert hasattr(lib, n), n
    assert sorted(abi.functions) == names          # two independent readings of the header
    for n in names:
        assert getattr(lib, n).argtypes == abi.functions[n][1] and getattr(lib, n).restype is abi.functions[n][0], n
    assert lib.dlsg_abi_version() == hip.ABI_VERSION == abi.defines['DLSG_ABI_VERSION'] == 8


def test_struct_layouts_match_the_compiler():
    lib = hip.load_library()
    assert len(STRUCT_INDEX) == 31 and sorted(STRUCT_INDEX + ['dlsg_gemm_group']) == sorted(abi.structs)
    for i, name in enumerate(STRUCT_INDEX):
        assert lib.dlsg_struct_size(i) == ctypes.sizeof(abi.structs[name]), name
    assert lib.dlsg_struct_size(99) == -1


def test_member_offsets_match_the_host_compiler(tmp_path):
    """The header compiled by the host C compiler: sizeof of every struct, offsetof and sizeof of every member, against the
    ctypes classes abi.py built from the same text.  Two members of equal size swapped in either reading, or an int32 taken for
    an int64, would pass the size check above and fail here."""
    cc = shutil.which('cc')
    if cc is None:
        pytest.skip('no host C compiler (cc) on PATH')
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "dlsg.h"', 'int main(void) {']
    want = []
    for name, st in abi.structs.items():
        src.append('    printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        want.append('%s %d' % (name, ctypes.sizeof(st)))
        for field, _ in st._fields_:
            src.append('    printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (name, field, name, field, name, field))
            want.append('%s.%s %d %d' % (name, field, getattr(st, field).offset, getattr(st, field).size))
    src += ['    return 0;', '}', '']
    (tmp_path / 'layout.c').write_text('\n'.join(src))
    subprocess.check_call([cc, '-std=c99', '-I', os.path.join(ROOT, 'include'), '-o', str(tmp_path / 'layout'), str(tmp_path / 'layout.c')])
    got = subprocess.check_output([str(tmp_path / 'layout')]).decode().split('\n')[:-1]
    assert len(want) > 500
    assert [g for g, w in zip(got, want) if g != w] == [] and len(got) == len(want)


# ---------------------------------------------------------------- the parser, construct by construct
def layout(st):
    return [(n, getattr(st, n).offset, getattr(st, n).size) for n, _ in st._fields_]


def test_parser_defines():
    d = abi.parse('''
        #ifndef X_H
        #define X_H
        #include <stdint.h>
        #define DLSG_A 8 /* comment */
        #define DLSG_NEG (-3)   // another
        #define DLSG_B (DLSG_A * 2 + 1)
        #define DLSG_SHIFT (1 << DLSG_A)
        #define DLSG_NAME "text"
        #define DLSG_F 1.5
        #define DLSG_CALL(x) (x)
        #endif''')[0]
    assert d == {'DLSG_A': 8, 'DLSG_NEG': -3, 'DLSG_B': 17, 'DLSG_SHIFT': 256}


def test_parser_struct_members():
    assert ctypes.sizeof(ctypes.c_void_p) == 8
    _, s, _ = abi.parse('''
        #define DLSG_N 4
        typedef struct {
            const float* A; float* const B;   /* const on either side, two declarations on a line */
            int64_t lda, ldb;                 /* several declarators */
            int32_t K; uint32_t site; float p; double d; uint64_t seed; int n;
            const uint64_t* seed_ptr; void* ws;
        } dlsg_inner;
        typedef struct {
            dlsg_inner f;                     /* a struct by value */
            dlsg_inner g[DLSG_N];             /* an array of structs, bound by a define */
            float* dKp[2]; const float* dy[3][DLSG_N]; int32_t n[4], m;
            const dlsg_inner* link;
        } dlsg_outer;''')
    assert list(s) == ['dlsg_inner', 'dlsg_outer']
    assert layout(s['dlsg_inner']) == [('A', 0, 8), ('B', 8, 8), ('lda', 16, 8), ('ldb', 24, 8), ('K', 32, 4), ('site', 36, 4), ('p', 40, 4),
                                       ('d', 48, 8), ('seed', 56, 8), ('n', 64, 4), ('seed_ptr', 72, 8), ('ws', 80, 8)]
    kinds = dict(s['dlsg_inner']._fields_)
    assert (kinds['A'], kinds['K'], kinds['site'], kinds['p'], kinds['d'], kinds['seed'], kinds['n'], kinds['lda']) == (
        ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32, ctypes.c_float, ctypes.c_double, ctypes.c_uint64, ctypes.c_int, ctypes.c_int64)
    assert layout(s['dlsg_outer']) == [('f', 0, 88), ('g', 88, 352), ('dKp', 440, 16), ('dy', 456, 96), ('n', 552, 16), ('m', 568, 4),
                                       ('link', 576, 8)]
    o = dict(s['dlsg_outer']._fields_)
    assert o['f'] is s['dlsg_inner'] and o['g']._type_ is s['dlsg_inner'] and o['g']._length_ == 4
    assert o['dy']._length_ == 3 and o['dy']._type_._length_ == 4 and o['dy']._type_._type_ is ctypes.c_void_p
    assert o['link'] is ctypes.POINTER(s['dlsg_inner'])


def test_parser_prototypes():
    _, s, f = abi.parse('''
        #ifdef __cplusplus
        extern "C" {
        #endif
        typedef struct { int32_t n; } dlsg_a;
        typedef struct dlsg_comm dlsg_comm;   /* opaque: no struct is built */
        int dlsg_version(void);
        int64_t dlsg_bytes(int B, int64_t ld);
        int dlsg_run(const dlsg_a* a, int count, float p, uint64_t seed, uint32_t site, double s, const int64_t* ids,
                     void* stream);           /* broken over lines */
        int dlsg_init(dlsg_comm** out, const void* id, int32_t* world, const dlsg_comm* c, float* const* grads);
        #ifdef __cplusplus
        }
        #endif''')
    vp = ctypes.c_void_p
    assert list(s) == ['dlsg_a']
    assert f == {'dlsg_version': (ctypes.c_int, []),
                 'dlsg_bytes': (ctypes.c_int64, [ctypes.c_int, ctypes.c_int64]),
                 'dlsg_run': (ctypes.c_int, [ctypes.POINTER(s['dlsg_a']), ctypes.c_int, ctypes.c_float, ctypes.c_uint64, ctypes.c_uint32,
                                             ctypes.c_double, vp, vp]),
                 'dlsg_init': (ctypes.c_int, [vp, vp, vp, vp, vp])}


@pytest.mark.parametrize('text, line', [
    ('typedef struct {\n    int32_t n;\n    unsigned int m;\n} dlsg_a;', 3),          # a type outside the subset
    ('typedef struct {\n    int32_t n;\n\n    size_t m;\n} dlsg_a;', 4),              # an unknown type
    ('typedef struct {\n    float (*fn)(int);\n} dlsg_a;', 2),                         # a function pointer
    ('typedef struct {\n    int32_t n[DLSG_MISSING];\n} dlsg_a;', 2),                  # a bound no define gives
    ('typedef struct {\n    int32_t n : 3;\n} dlsg_a;', 2),                            # a bit field
    ('typedef struct {\n    int32_t;\n} dlsg_a;', 2),                                  # no member name
    ('/* c */\nint dlsg_f(int a,\n           long b);', 2),                             # an unknown parameter type
    ('int dlsg_f(int a);\nvoid dlsg_g(int a);', 2),                                     # a return type a binding cannot check
    ('int dlsg_f(int a);\n\nstruct dlsg_x { int a; };', 3),                             # a construct outside the subset
])
def test_parser_refuses_what_it_does_not_know(text, line):
    with pytest.raises(ValueError, match=r'line %d\b' % line):
        abi.parse(text)


def test_missing_header_names_the_path(tmp_path):
    """a package copied without include/dlsg.h fails at import and says where it looked"""
    import sys
    pkg = tmp_path / 'pkg' / 'lonely'
    pkg.mkdir(parents=True)
    (pkg / '__init__.py').write_text('')
    shutil.copy(abi.__file__, str(pkg / 'abi.py'))
    r = subprocess.run([sys.executable, '-c', 'import lonely.abi'], cwd=str(tmp_path / 'pkg'), stderr=subprocess.PIPE)
    assert r.returncode != 0 and str(tmp_path / 'include' / 'dlsg.h') in r.stderr.decode()


def test_product_path_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    with pytest.raises(RuntimeError):
        hip.HipOps()
    import dlsg_amd
    from helpers import small_args
    net = dlsg_amd.CapGnnModel(small_args(), dlsg_amd.make_vocab(50))
    with pytest.raises(RuntimeError):
        net(torch.zeros(1, 26, 112), torch.zeros(1, 26, 16, 32), torch.zeros(1, 26, dtype=torch.long))


def test_integration_doc_names_every_entry_point():
    """INTEGRATION.md is the reference-side binding guide: every symbol include/dlsg.h declares must appear in it."""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'dlsg.h')).read()
    doc = open(os.path.join(root, 'INTEGRATION.md')).read()
    names = sorted(set(re.findall(r'\b(dlsg_[a-z0-9_]+)\s*\(', header)))
    missing = []
    for n in names:
        stem = re.sub(r'_(fwd|bwd)$', '', n)
        if n not in doc and (stem + '_fwd/bwd') not in doc:
            missing.append(n)
    assert not missing, missing
