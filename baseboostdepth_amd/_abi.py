"""Reader of include/bbd_hip.h: the prototypes and the BBD_* constants of the C ABI, as `ctypes` needs them.

The header is the one description of the ABI; `_lib.py` and the host-port binding of the tests type every call from what
this module reads.  It is no C parser: the header keeps to `int` / `long` results, to `int`, `long`, `unsigned` and `double`
by value and to pointers, and to defines whose value is one integer literal.  Anything else raises - a header this reader
does not understand stops the import, as a missing library does.
"""
import collections
import ctypes
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bbd_hip.h")


class BbdError(RuntimeError):
    pass


# params = ((ctypes type, name), ...), `void* stream` included; has_stream: the last parameter is `void* stream`
Prototype = collections.namedtuple("Prototype", "restype params has_stream")

_BY_VALUE = {"int": ctypes.c_int, "long": ctypes.c_long, "unsigned": ctypes.c_uint, "double": ctypes.c_double}
_PROTOTYPE = re.compile(r"([^;{}()]*?)\b(bbd_\w+)\s*\(([^()]*)\)\s*;")
_DEFINE = re.compile(r"#[ \t]*define[ \t]+(BBD_\w+)(.*)")
_INTEGER = re.compile(r"-?(?:0[xX][0-9a-fA-F]+|[1-9][0-9]*|0)")


def _parameter(function, text):
    text = " ".join(text.split())
    if "*" in text:
        return ctypes.c_void_p, re.search(r"(\w*)$", text).group(1)
    spelling, _, name = text.rpartition(" ")
    if spelling not in _BY_VALUE:
        raise BbdError("%s: parameter `%s` is neither a pointer nor int, long, unsigned or double by value" % (function, text))
    return _BY_VALUE[spelling], name


def parse(text):
    """(prototypes, constants) of header text: {"bbd_name": Prototype} in the header's order, {"NAME": value} for every
    `#define BBD_NAME <integer literal>` (decimal, hex or a parenthesised negative)."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    constants, code = {}, []
    for line in text.splitlines():
        if not line.lstrip().startswith("#"):
            code.append(line)
            continue
        define = _DEFINE.match(line.strip())
        if define and define.group(2).strip():                  # an empty right-hand side: the include guard
            macro, value = define.group(1), define.group(2).strip()
            if value[0] == "(" and value[-1] == ")":
                value = value[1:-1].strip()
            if define.group(2)[0] not in " \t" or not _INTEGER.fullmatch(value):
                raise BbdError("%s: the value `%s` is not one integer literal" % (macro, define.group(2).strip()))
            constants[macro[len("BBD_"):]] = int(value, 0)
    prototypes = {}
    for result, function, params in _PROTOTYPE.findall("\n".join(code)):
        if result.strip() not in ("int", "long"):
            raise BbdError("%s: the result `%s` is neither int nor long" % (function, result.strip()))
        params = () if params.strip() in ("", "void") else tuple(_parameter(function, p) for p in params.split(","))
        streams = [i for i, p in enumerate(params) if p[1] == "stream"]
        if streams not in ([], [len(params) - 1]) or (streams and params[-1][0] is not ctypes.c_void_p):
            raise BbdError("%s: `stream` must be the last parameter and a void*" % function)
        prototypes[function] = Prototype(_BY_VALUE[result.strip()], params, bool(streams))
    return prototypes, constants


def read_header(path=HEADER):
    if not os.path.isfile(path):
        raise BbdError("C-ABI header %s not found - the Python binding is read from it. There is no CPU fallback." % path)
    with open(path) as f:
        return parse(f.read())
