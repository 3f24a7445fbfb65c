"""tests/test_gpu_streams.py stays complete against include/jat_hip.h: every function that takes a `void* stream` is run by a
side-stream case or listed in EXEMPT with a reason, every name in the tables is such a function, and the entries documented as
never synchronising stay out of SYNCHRONISES.  No GPU: importing the case table builds no case."""
import os
import re

import test_gpu_streams as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declarations(header_text):
    """[(name, argument text)] of every function the header declares"""
    text = re.sub(r"/\*.*?\*/", " ", header_text, flags=re.S)
    return re.findall(r"\b(?:int|void|const char\s*\*)\s*(jat_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S)


def stream_entries(header_text):
    """names of the functions declared with a `void* stream` parameter"""
    return [name for name, args in declarations(header_text) if re.search(r"\bvoid\s*\*\s*stream\b", args)]


def header():
    with open(os.path.join(ROOT, "include", "jat_hip.h")) as f:
        return f.read()


def missing(entries, covered, exempt):
    return sorted(set(entries) - set(covered) - set(exempt))


def test_the_parser_finds_the_stream_taking_entries():
    e = stream_entries(header())
    assert len(e) == len(set(e)) and len(e) == 75, len(e)
    for name in ("jat_forward", "jat_k_dac_rvq", "jat_yin", "jat_bank_blend_topk", "jat_trainer_create", "jat_f0_compare"):
        assert name in e, name
    for name in ("jat_bank_create", "jat_bank_clear", "jat_solver_plan", "jat_k_gemm_plan", "jat_model_workspace_bytes"):
        assert name not in e, name


def test_every_stream_taking_entry_has_a_case_or_a_reason():
    e = stream_entries(header())
    assert missing(e, S.covered_entries(), S.EXEMPT) == []
    assert all(isinstance(r, str) and r.strip() for r in S.EXEMPT.values())
    assert not set(S.EXEMPT) & set(S.covered_entries()), "an exempt entry has a case: drop the exemption"


def test_a_deleted_case_is_noticed():
    """the check itself: without the only case that runs them, jat_k_gelu and jat_k_gelu_bwd are reported"""
    e = stream_entries(header())
    covered = {x for name, (covers, _) in S.CASES.items() if name != "k_gelu_and_gelu_bwd" for x in covers}
    assert missing(e, covered, S.EXEMPT) == ["jat_k_gelu", "jat_k_gelu_bwd"]


def test_the_tables_name_only_stream_taking_entries():
    e = set(stream_entries(header()))
    declared = {name for name, _ in declarations(header())}      # a case may also name what it runs that takes no stream
    assert len(declared) >= 130 and e < declared
    assert set(S.covered_entries()) <= declared, sorted(set(S.covered_entries()) - declared)
    assert set(S.EXEMPT) <= e and set(S.SYNCHRONISES) <= declared
    assert all(isinstance(r, str) and r.strip() for r in S.SYNCHRONISES.values())


def test_never_synchronise_entries_stay_out_of_the_table():
    S.test_the_never_synchronise_entries_are_not_in_the_table()
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        doc = f.read()
    for name in S.SYNCHRONISES:
        assert f"`{name}`" in doc, f"{name} synchronises: INTEGRATION.md's table must say so"
