"""The environment switches of the library, held to their one table (no GPU: the sources are read as text).

* every "OSQP_AMD_..." string literal in csrc/*.hip and *.hpp is documented in DESIGN.md section 9, by its full name or in the
  table's abbreviated form (`_SNODE_MAX` after an `OSQP_AMD_SNODE=...` in the same row);
* the direct back-end reads the environment in one place: direct.hip and the headers it includes hold no getenv( -- the parse
  helpers live in common.hpp -- and every switch of csrc/direct_knobs.hpp is named exactly once there and nowhere in them."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "osqp.jl_amd", "csrc")
LITERAL = re.compile(r'"(OSQP_AMD_[A-Z0-9_]+)"')


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _sources():
    return {f: _read(os.path.join(CSRC, f)) for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".hpp"))}


def _section9():
    text = _read(os.path.join(ROOT, "DESIGN.md"))
    start = text.index("\n## 9. ")
    return text[start:text.index("\n## 10. ", start)]


def _direct_sources():
    """direct.hip and every header of csrc it includes, directly or not; common.hpp, where the parse helpers live, left out."""
    src, seen, todo = _sources(), [], ["direct.hip"]
    while todo:
        f = todo.pop()
        if f in seen or f == "common.hpp" or f not in src:
            continue
        seen.append(f)
        todo += re.findall(r'#include "([^"/]+)"', src[f])
    return {f: src[f] for f in seen}


def test_every_switch_is_documented():
    doc = _section9()
    names = sorted({n for text in _sources().values() for n in LITERAL.findall(text)})
    assert len(names) > 80, names
    missing = [n for n in names
               if not re.search(r"(?:OSQP_AMD|(?<![A-Z0-9_]))" + re.escape(n[len("OSQP_AMD"):]) + r"(?![A-Z0-9_])", doc)]
    assert not missing, missing


def test_direct_backend_reads_the_environment_in_one_place():
    files = _direct_sources()
    assert {"direct.hip", "direct_knobs.hpp", "direct_sn_kernels.hpp", "mfront.hpp", "mfront_big.hpp", "direct_adjoint.hpp"} <= set(files)
    assert [f for f, text in files.items() if "getenv(" in text] == []
    knobs = LITERAL.findall(files["direct_knobs.hpp"])
    assert len(knobs) >= 40 and len(knobs) == len(set(knobs)), sorted(n for n in set(knobs) if knobs.count(n) > 1)
    elsewhere = {f: sorted(set(LITERAL.findall(text)) & set(knobs)) for f, text in files.items() if f != "direct_knobs.hpp"}
    assert not any(elsewhere.values()), elsewhere
