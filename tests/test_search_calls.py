"""The host layer of the search calls is pinned: what every argument form of BatchedJssEnv's fourteen search methods returns, the
class and the text of every exception they raise, the refusals of BucketedJssEnv and JssVectorEnv and the drivers' argument errors
and small runs, over the fixed list of tests/search_call_cases.py.  tests/golden/search_calls.json holds, per call, the shape,
dtype and SHA-256 of every returned array, or the exception; it was recorded with the CPU twin from the code as it stood before
the search calls moved into jssenv_amd/search_calls.py, and is not recorded again from code that claims to behave the same.
On the MI355X the same list gives the same file: integers, the same bits on every backend (the one float output, lookahead's
return, is a float64 quotient rounded once, which tests/test_lookahead.py holds to equality as well)."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "search_calls.json")
sys.path.insert(0, HERE)

import search_call_cases as K  # noqa: E402


@pytest.fixture(scope="module")
def twin():
    return K.twin_backend()


@pytest.fixture(scope="module")
def hip():
    from jssenv_amd.env import HipBackend
    be = HipBackend("cuda:0")
    assert be.lib.jss_backend() == b"hip:gfx950"
    return be


def compare(got):
    with open(GOLDEN) as f:
        want = json.load(f)
    assert list(got) == list(want), "the list of calls changed"
    differ = [name for name in want if got[name] != want[name]]
    for name in differ[:10]:
        print(f"--- {name}\nrecorded: {want[name]}\nnow:      {got[name]}")
    assert not differ, f"{len(differ)} of {len(want)} calls differ from the record, the first: {differ[0]}"
    assert sum("returns" in r for r in want.values()) > 120 and sum("raises" in r for r in want.values()) > 200


def test_recorded_twin(twin):
    compare(K.run(twin))


@pytest.mark.gpu
def test_recorded_gpu(hip):
    compare(K.run(hip))


def test_structure():
    """the search calls do not know the env module, and the wrappers' refusals are the one table's"""
    import ast
    from jssenv_amd import BatchedJssEnv, BucketedJssEnv, JssVectorEnv, search_calls
    with open(search_calls.__file__) as f:
        tree = ast.parse(f.read())
    imported = set()
    for node in ast.walk(tree):                                          # (function-local imports too)
        if isinstance(node, ast.Import):
            imported |= {a.name for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            imported |= {node.module or "."} | ({a.name for a in node.names} if node.module is None else set())
    assert "_abi" in imported and not any(name.split(".")[-1] in ("env", "search") for name in imported), imported
    assert tuple(row[0] for row in search_calls.REFUSALS) == K.REFUSED and len(search_calls.LIBRARIES) == 10
    assert issubclass(BatchedJssEnv, search_calls.SearchCalls)
    for cls in (BucketedJssEnv, JssVectorEnv):
        for name, does_not, hint in search_calls.REFUSALS:
            assert getattr(cls, name).__module__ == "jssenv_amd.search_calls"
            with pytest.raises(NotImplementedError) as e:
                getattr(object.__new__(cls), name)()
            assert str(e.value) == f"{cls.__name__} {does_not}: call {name} on a BatchedJssEnv ({hint})"


if __name__ == "__main__":           # python tests/test_search_calls.py: records tests/golden/search_calls.json with the CPU twin
    got = K.run(K.twin_backend())
    with open(GOLDEN, "w") as f:
        json.dump(got, f, indent=0, sort_keys=False)
        f.write("\n")
    print(len(got), "calls ->", GOLDEN)
