"""tests/fp16_matrix.py stays complete and true to the files it names: every tests/test_gpu_*.py has an entry, every named test
exists, and every word of a `-k` expression occurs in a test id of its file (so a renamed test cannot empty a selection unseen).
No GPU: the ids come from one `pytest --collect-only` of the files with a `-k` selection, which only imports them."""
import glob
import os
import re
import subprocess
import sys

import pytest

import fp16_matrix as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")


def test_every_gpu_file_has_an_entry_and_every_entry_a_file():
    on_disk = sorted(os.path.basename(p) for p in glob.glob(os.path.join(TESTS, "test_gpu_*.py")))
    assert on_disk == sorted(M.MATRIX), (sorted(set(on_disk) - set(M.MATRIX)), sorted(set(M.MATRIX) - set(on_disk)))
    for name, entry in M.MATRIX.items():
        assert isinstance(entry, tuple) and len(entry) == 2 and entry[0] in M.KINDS, name
        kind, what = entry
        if kind == "child":
            assert what and all(isinstance(a, list) and all(isinstance(x, str) for x in a) for a in what), name
            assert all(a == [] or (len(a) == 2 and a[0] == "-k") for a in what), name
        else:
            assert isinstance(what, str) and what.strip() and "\n" not in what, name
    ids = [i for i, _ in M.children()]
    assert len(set(ids)) == len(ids)


def test_every_named_test_exists_in_its_file():
    named = [(name, what) for name, (kind, what) in M.MATRIX.items() if kind in ("same_bits", "own_child")]
    assert named
    for name, test in named:
        with open(os.path.join(TESTS, name)) as f:
            assert re.search(r"^def %s\(" % re.escape(test), f.read(), re.M), (name, test)


@pytest.fixture(scope="module")
def collected():
    """file name -> the ids `test_name[params]` pytest collects from it, for the files with a `-k` selection"""
    files = sorted({args[0] for _, args in M.children() if "-k" in args})
    out = subprocess.run([sys.executable, "-m", "pytest", "--collect-only", "-q", "-p", "no:cacheprovider"] + files, cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    ids = {os.path.basename(f): [] for f in files}
    for line in out.stdout.splitlines():
        if "::" in line:
            path, rest = line.split("::", 1)
            ids[os.path.basename(path)].append(rest)
    return ids


def test_every_word_of_a_k_expression_occurs_in_a_test_id_of_its_file(collected):
    checked = 0
    for _, args in M.children():
        name = os.path.basename(args[0])
        for word in M.k_words(args):
            assert collected[name], name
            assert any(word.lower() in i.lower() for i in collected[name]), (name, word)
            assert word.lower() not in name.lower(), f"{word!r} is part of {name}: it selects the whole file"
            checked += 1
    assert checked > 20
