"""Reads include/cpn_hip.h: the one statement of the C ABI.  Standard library only.

``parse(text)`` -> ``Header(prototypes, structs, constants)``:

* ``prototypes``: name -> (restype, [argtypes]) of every ``cpn_*`` function, in header order;
* ``structs``: name -> ``ctypes.Structure`` class of every ``typedef struct { ... } name;`` (pointer fields are ``c_void_p``);
* ``constants``: ``CPN_X`` -> int of every integer ``#define`` and every enumerator.

Strict: a statement, field or ``CPN_`` macro it cannot map completely raises ``ValueError`` naming it; nothing is skipped
silently.  Macros without a value (the include guard, ``CPN_HOST``) define no constant.

Pointers.  A pointer to void, to a scalar or to the opaque ``cpn_plan`` is ``c_void_p``: an address, device memory as a rule.
``CPN_HOST`` in front of a parameter, or an array declarator (``int32_t info[5]``, always host memory), makes a pointer to a scalar
``POINTER(T)``, so that ctypes rejects a host buffer of another element type.  A pointer to a pointer is a host array of
addresses, ``POINTER(c_void_p)``; a pointer to a struct of the header is ``POINTER(Struct)``.
"""
import collections
import ctypes
import os
import re
from ctypes import POINTER, c_void_p

HEADER_PATH = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'cpn_hip.h'))

SCALARS = {'int': ctypes.c_int32, 'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'float': ctypes.c_float,
           'double': ctypes.c_double, 'size_t': ctypes.c_size_t, 'uint32_t': ctypes.c_uint32, 'uint8_t': ctypes.c_uint8,
           'unsigned long long': ctypes.c_uint64}

Header = collections.namedtuple('Header', 'prototypes structs constants')
_INT = r'(-?(?:0[xX][0-9a-fA-F]+|\d+))'
_BASE = re.compile(r'(unsigned long long|\w+)\b(.*)$', re.S)
_DECLARATOR = re.compile(r'^([\s*]*)(\w*)\s*(\[\d*\])?\s*$')
_HOST = re.compile(r'\bCPN_HOST\b')
_CALLED = re.compile(r'\bcpn_\w+(?=\s*\()')
_PROTOTYPE = re.compile(r'^([\w\s*]+?)\b(cpn_\w+) ?\(([^()]*)\)$')


def _declarations(text, structs, opaque, where, in_struct=False):
    """``text`` = one parameter or one field declaration, possibly with several declarators -> [(name, ctype)]."""
    text, host = _HOST.subn(' ', text)
    m = _BASE.match(text.strip())
    if not m or not (m.group(1) in SCALARS or m.group(1) in structs or m.group(1) in opaque or m.group(1) in ('void', 'char')):
        raise ValueError(f'{where}: unknown type in "{text}"')
    base, out = m.group(1), []
    for decl in m.group(2).split(','):
        d = _DECLARATOR.match(decl)
        if not d or (in_struct and not d.group(2)):
            raise ValueError(f'{where}: cannot read the declarator "{decl.strip()}" of "{text}"')
        levels = d.group(1).count('*') + bool(d.group(3))
        if levels == 0 and base in SCALARS:
            ctype = SCALARS[base]
        elif levels == 1 and base in structs and not in_struct:
            ctype = POINTER(structs[base])
        elif levels == 1 and base in SCALARS and (host or d.group(3)) and not in_struct:
            ctype = POINTER(SCALARS[base])
        elif levels == 1 and base != 'char' or (levels == 2 and in_struct):
            ctype = c_void_p
        elif levels == 2:
            ctype = POINTER(c_void_p)
        else:
            raise ValueError(f'{where}: no ctypes type for "{text}"')
        out.append((d.group(2), ctype))
    return out


def _restype(text, where):
    text = text.strip()
    if text in SCALARS:
        return SCALARS[text]
    if text in ('void', 'char *'):
        return None if text == 'void' else ctypes.c_char_p
    raise ValueError(f'{where}: unknown return type "{text}"')


def parse(text):
    text = re.sub(r'/\*.*?\*/|//[^\n]*|\bconst\b', ' ', text, flags=re.S)  # comments; const changes no type here
    prototypes, structs, constants, opaque = {}, {}, {}, set()
    lines = []
    for line in text.split('\n'):  # preprocessor lines: constants out, everything else of them dropped
        if not line.lstrip().startswith('#'):
            lines.append(line)
            continue
        m = re.match(r'\s*#\s*define\s+(\w+)\s*(.*?)\s*$', line)
        if m and m.group(2):
            v = re.match(r'^(?:%s|\(\s*%s\s*\))$' % (_INT, _INT), m.group(2))
            if not v or not m.group(1).startswith('CPN_'):
                raise ValueError(f'#define {m.group(1)}: cannot read the value "{m.group(2)}"')
            constants[m.group(1)] = int(v.group(1) or v.group(2), 0)
        elif not m and not re.match(r'\s*#\s*(include|ifdef|ifndef|endif)\b', line):
            raise ValueError(f'cannot read the preprocessor line "{line.strip()}"')
    text, wrapped = re.subn(r'extern\s+"C"\s*\{', ' ', '\n'.join(lines))
    statements, depth, start = [], 0, 0
    for m in re.finditer(r'[{};]', text):  # statements end at a ';' outside braces
        depth += (m.group(0) == '{') - (m.group(0) == '}')
        if m.group(0) == ';' and depth == 0:
            statements.append(' '.join(text[start:m.start()].split()))
            start = m.end()
    tail = text[start:].strip()
    if tail != '}' * wrapped:
        called = _CALLED.search(tail)
        raise ValueError(f'{called.group(0) if called else "header"}: unterminated text "{tail[:80]}"')
    for st in statements:
        called = _CALLED.search(st)
        m = re.match(r'^typedef struct (\w+ )?\{(.*)\} (\w+)$', st)
        if m:
            name, fields = m.group(3), []
            for field in filter(None, (f.strip() for f in m.group(2).split(';'))):
                fields += _declarations(field, structs, opaque, f'struct {name}', in_struct=True)
            structs[name] = type(name, (ctypes.Structure,), {'_fields_': fields})
        elif re.match(r'^typedef struct (\w+) \1$', st):
            opaque.add(st.split()[-1])
        elif re.match(r'^enum \{.*\}$', st):
            value = -1
            for item in st[st.index('{') + 1:-1].split(','):
                m = re.match(r'^\s*(CPN_\w+)\s*(?:=\s*%s)?\s*$' % _INT, item)
                if not m:
                    raise ValueError(f'enum: cannot read the enumerator "{item.strip()}"')
                value = int(m.group(2), 0) if m.group(2) else value + 1
                constants[m.group(1)] = value
        elif called:
            name = called.group(0)
            m = _PROTOTYPE.match(st)
            if not m or m.group(2) != name or name in prototypes:
                raise ValueError(f'{name}: cannot read the declaration "{st}"')
            params = [] if m.group(3).strip() == 'void' else m.group(3).split(',')
            argtypes = []
            for i, p in enumerate(params):
                got = _declarations(p, structs, opaque, f'{name}, parameter {i + 1}')
                if len(got) != 1:
                    raise ValueError(f'{name}, parameter {i + 1}: cannot read "{p.strip()}"')
                argtypes.append(got[0][1])
            prototypes[name] = (_restype(m.group(1), name), argtypes)
        else:
            raise ValueError(f'cannot read the statement "{st[:80]}"')
    return Header(prototypes, structs, constants)


_header = None


def header():
    """The parsed include/cpn_hip.h of this tree (parsed once per process)."""
    global _header
    if _header is None:
        if not os.path.isfile(HEADER_PATH):
            raise RuntimeError(f'{HEADER_PATH} not found: the binding is derived from it.')
        with open(HEADER_PATH) as f:
            _header = parse(f.read())
    return _header
