"""include/adroit_wave.h as data: the one parser the tests of the C-ABI share.  Pure functions of the
header's text (comments stripped, whitespace normalised); nothing is compiled or loaded."""
import functools
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "adroit_wave.h")


@functools.lru_cache(maxsize=None)
def text() -> str:
    """the header's text without its comments"""
    with open(HEADER) as f:
        src = f.read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    return src


def _norm(s: str) -> str:
    return re.sub(r"\s+", " ", s).strip()


def prototypes() -> dict:
    """{function name: (return type, [parameter declarations])} in the header's order; ``(void)`` is
    an empty list.  e.g. "aw_destroy": ("int", ["aw_handle* h"])"""
    out = {}
    for ret, name, params in re.findall(r"^\s*(int|const char\*)\s+(aw_\w+)\s*\(([^)]*)\)\s*;", text(), re.M):
        params = _norm(params)
        out[name] = (ret, [] if params in ("", "void") else [_norm(p) for p in params.split(",")])
    return out


def defines() -> dict:
    """{name: value} of the integer ``#define AW_*``"""
    return {k: int(v, 0) for k, v in re.findall(r"^\s*#define\s+(AW_\w+)\s+(-?(?:0[xX][0-9a-fA-F]+|\d+))\s*$", text(), re.M)}


def enums() -> dict:
    """{enumerator: value} of every enum of the header (an enumerator without ``= value`` is its
    predecessor's plus one, the first 0)"""
    out = {}
    for body in re.findall(r"\benum\s*\{([^}]*)\}", text()):
        nxt = 0
        for item in body.split(","):
            item = _norm(item)
            if not item:
                continue
            name, _, val = (x.strip() for x in item.partition("="))
            nxt = int(val, 0) if val else nxt
            out[name] = nxt
            nxt += 1
    return out


def struct_body(name: str) -> str:
    """the text between the braces of ``typedef struct { ... } name;``, whitespace normalised"""
    m = re.search(r"typedef struct \{([^}]*)\}\s*%s\s*;" % re.escape(name), text())
    assert m, f"no struct {name} in the header"
    return _norm(m.group(1))


def struct_fields(name: str) -> list:
    """[(type, field name)] of ``typedef struct { ... } name;`` in declaration order; a pointer's
    stars belong to the type ("float*"), an array's extent stays on the name ("rec[AW_CAM_FLOATS]")"""
    out = []
    for decl in struct_body(name).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        first, *rest = [x.strip() for x in decl.split(",")]
        m = re.match(r"(.*?)([\w\[\]]+)$", first)
        base, stars = re.match(r"([^*]*?)\s*(\**)\s*$", m.group(1)).groups()
        out.append((_norm(base) + stars, m.group(2)))
        for item in rest:
            s, field = re.match(r"(\**)\s*([\w\[\]]+)$", item).groups()
            out.append((_norm(base) + s, field))
    return out
