"""The C ABI of libdlsg_hip.so, read from include/dlsg.h: the header is the only place that writes the layout down.

`parse` understands the small, regular subset of C the header is written in and nothing else; whatever it does not
recognise is an error that names the line, never a skipped declaration (a dropped struct member would shift every field
behind it).  The module parses the header once, when it is imported, and offers

  defines    {'DLSG_ABI_VERSION': 8, 'DLSG_GEMM_ACCUM': 1, ...}   every #define with an integer value
  structs    {'dlsg_gemm_args': <ctypes.Structure subclass>, ...}  also module attributes: abi.dlsg_gemm_args
  functions  {'dlsg_gemm': (restype, [argtypes]), ...}
  extensions {'dlsg_sample_ens': (restype, [argtypes])}            the prototypes of the headers beside dlsg.h (EXTENSION_HEADERS)
  addons     {'dlsg_risk_rows': (restype, [argtypes]), ...}        the prototypes of include/addons/*.h, read in sorted order

Types: the fixed-width integers, int, float and double map to their ctypes scalars; a pointer to a struct of the header
is POINTER(that struct); every other pointer is c_void_p.
"""
import ctypes as C
import os
import re

HEADER = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..', 'include', 'dlsg.h'))

SCALARS = {'int32_t': C.c_int32, 'int64_t': C.c_int64, 'uint16_t': C.c_uint16, 'uint32_t': C.c_uint32, 'uint64_t': C.c_uint64,
           'float': C.c_float, 'int': C.c_int, 'double': C.c_double}

# one top-level item of the header, after comments are blanked
_ITEM = re.compile(r'''\s*(?:
      \#\s*define\s+(?P<define>\w+)[ \t]*(?P<value>[^\n]*)
    | \#[^\n]* | extern\s*"C"\s*\{ | \}
    | typedef\s+struct\s+(?P<opaque>\w+)\s+(?P=opaque)\s*;
    | typedef\s+struct\s*\{(?P<body>[^{}]*)\}\s*(?P<struct>\w+)\s*;
    | (?P<ret>\w+)\s+(?P<func>\w+)\s*\((?P<params>[^()]*)\)\s*;
    )''', re.X)
# [const] base [const] {* [const]} [name] {[bound]}
_DECL = re.compile(r'(?:const\s+)?(\w+)(?:\s+const)?\s*((?:\*\s*(?:const\s*)?)*)(\w*)\s*((?:\[\s*\w+\s*\])*)$')


def parse(text):
    """(defines, structs, functions) of a header given as a string"""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', lambda m: '\n' * m.group(0).count('\n'), text, flags=re.S)
    defines, structs, functions, opaque = {}, {}, {}, set()

    def fail(pos, what):
        raise ValueError('dlsg.h line %d: cannot parse %r' % (text.count('\n', 0, pos) + 1, ' '.join(what.split())))

    def declarator(decl, pos, base=None):
        """'const float* dy[3][DLSG_CLN_MAXG]' -> (base type name, field name, ctype)"""
        m = _DECL.match(decl if base is None else base + ' ' + decl)
        if not m:
            fail(pos, decl)
        base, stars, name, bounds = m.group(1), m.group(2).count('*'), m.group(3), re.findall(r'\w+', m.group(4))
        if base in structs:
            t = (structs[base], C.POINTER(structs[base]))[stars] if stars < 2 else C.c_void_p
        elif stars and (base in SCALARS or base in opaque or base == 'void'):
            t = C.c_void_p
        elif not stars and base in SCALARS:
            t = SCALARS[base]
        else:
            fail(pos, decl)
        for b in reversed(bounds):
            if not (b.isdigit() or b in defines):
                fail(pos, decl)
            t = t * (int(b) if b.isdigit() else defines[b])
        return base, name, t

    pos, end = 0, len(text.rstrip())
    while pos < end:
        m = _ITEM.match(text, pos)
        if not m:
            rest = text[pos:].lstrip()
            fail(len(text) - len(rest), rest.split('\n')[0])
        if m.group('define') and re.fullmatch(r'[\w\s()+\-*|&<>~]+', m.group('value')):
            try:
                value = eval(m.group('value'), {'__builtins__': {}}, dict(defines))  # integer expressions of earlier defines
            except (NameError, SyntaxError, TypeError):
                value = None
            if isinstance(value, int):
                defines[m.group('define')] = value
        elif m.group('opaque'):
            opaque.add(m.group('opaque'))
        elif m.group('struct'):
            fields, at = [], m.start('body')
            for member in m.group('body').split(';'):
                here = at + len(member) - len(member.lstrip())   # where this member's text starts: the line an error names
                at += len(member) + 1
                base = None
                for d in member.split(',') if member.strip() else ():
                    base, name, t = declarator(d.strip(), here, base)
                    if not name:
                        fail(here, member)
                    fields.append((name, t))
            structs[m.group('struct')] = type(m.group('struct'), (C.Structure,), {'_fields_': fields})
        elif m.group('func'):
            params = m.group('params').strip()
            if m.group('ret') not in ('int', 'int64_t'):
                fail(m.start('ret'), m.group(0))
            functions[m.group('func')] = (SCALARS[m.group('ret')],
                                          [declarator(p.strip(), m.start('params'))[2] for p in params.split(',')]
                                          if params not in ('', 'void') else [])
        pos = m.end()
    return defines, structs, functions


if not os.path.exists(HEADER):
    raise RuntimeError('include/dlsg.h not found (%s): dlsg_amd reads the C ABI of libdlsg_hip.so from it' % HEADER)
with open(HEADER) as _f:
    defines, structs, functions = parse(_f.read())
globals().update(structs)

# Entry points beside the versioned ABI: dlsg.h's list is what DLSG_ABI_VERSION counts; an addition that changes no existing entry point
# stands in a header of its own next to it, in the same subset of C (prototypes only: no struct, no define), and is read the same way.
EXTENSION_HEADERS = ('dlsg_sample_ens.h',)
extensions = {}
for _name in EXTENSION_HEADERS:
    with open(os.path.join(os.path.dirname(HEADER), _name)) as _f:
        _d, _s, _fn = parse(_f.read())
    if _d or _s or set(_fn) & (set(functions) | set(extensions)):
        raise RuntimeError('include/%s: an extension header declares new prototypes only' % _name)
    extensions.update(_fn)


# Every later entry point: one header per addition under include/addons/, prototypes only, read in sorted order.  A test pins the names
# it owns ({'dlsg_x'} <= set(abi.addons)), never a total, so an addition leaves every earlier pin alone.
ADDONS_DIR = os.path.join(os.path.dirname(HEADER), 'addons')


def read_addons(directory, taken):
    """{name: (restype, [argtypes])} of the *.h under `directory`; a struct, an integer #define, or a name in `taken` or in an earlier
    addon header is an error that names the header and the line"""
    out = {}
    for name in sorted(os.listdir(directory)) if os.path.isdir(directory) else ():
        if not name.endswith('.h'):
            continue
        with open(os.path.join(directory, name)) as f:
            text = f.read()
        d, s, fn = parse(text)

        bare = re.sub(r'/\*.*?\*/|//[^\n]*', lambda c: '\n' * c.group(0).count('\n'), text, flags=re.S)   # (comments blanked, lines kept)

        def line_of(word):
            return bare.count('\n', 0, re.search(r'\b%s\b' % re.escape(word), bare).start()) + 1

        for word in list(d) + list(s):
            raise ValueError('include/addons/%s line %d: %s -- an addon header declares prototypes only' % (name, line_of(word), word))
        for word in fn:
            if word in taken or word in out:
                raise ValueError('include/addons/%s line %d: %s is already declared' % (name, line_of(word), word))
        out.update(fn)
    return out


addons = read_addons(ADDONS_DIR, set(functions) | set(extensions))
