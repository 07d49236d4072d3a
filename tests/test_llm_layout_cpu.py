"""The layering of the LLaMA path's Python: llm_laws <- llm_engine <- minigpt4.  Every name keeps its old address in
`certifiedgpt_amd.minigpt4` (the same object as in its new home), the laws import nothing of the package and no ctypes, and the
classifier stays defined in minigpt4.py, where the CPU tests replace the engine it resolves through the module's globals."""
import ast
import inspect

import pytest

from certifiedgpt_amd import llm_engine, llm_laws, minigpt4

LAWS = ["MAX_STOP_SEQS", "MAX_STOP_LEN", "_as_rows", "stop_finish_columns", "apply_stop_sequences", "check_stop_words_ids",
        "stop_sequences_criteria",
        "PHILOX_WORD_SAMPLE", "SAMPLE_FIELDS", "SAMPLE_HF_DEFAULTS", "_philox4x32_10", "sample_uniform", "sample_token_law",
        "check_sample_settings",
        "greedy_decode_parity", "fp16_ulp",
        "LAYER_LINEARS", "quantize_rows_int8", "dequantize_rows_int8", "int8_state_dict", "quantize_act_rows_int8", "llm_int8_linear",
        "_ActInt8Linear", "act_int8_twin",
        "GQA_RATIOS", "expand_kv_state_dict",
        "left_pad_embeds", "pack_row_candidates"]
ENGINE = ["hip_decode_unsupported", "_rope_theta", "_HipDecoder", "_LinearRoute"]
STAYS = ["IMAGE_PLACEHOLDER", "prepare_texts", "clean_answer", "WordHashTokenizer", "MiniGPT4Classifier"]


@pytest.mark.parametrize("home, name", [(llm_laws, n) for n in LAWS] + [(llm_engine, n) for n in ENGINE])
def test_a_moved_name_is_the_same_object_at_its_old_address(home, name):
    assert getattr(minigpt4, name) is getattr(home, name)


def test_what_stays_is_defined_in_minigpt4():
    for name in STAYS:
        assert hasattr(minigpt4, name) and not hasattr(llm_laws, name) and not hasattr(llm_engine, name), name
    assert inspect.getmodule(minigpt4.MiniGPT4Classifier) is minigpt4
    assert inspect.getmodule(minigpt4.WordHashTokenizer) is minigpt4


def test_the_laws_import_nothing_of_the_package_and_no_ctypes():
    tree = ast.parse(inspect.getsource(llm_laws))
    modules = []
    for node in ast.walk(tree):                                        # the lazy imports inside function bodies too
        if isinstance(node, ast.Import):
            modules += [a.name for a in node.names]
        elif isinstance(node, ast.ImportFrom):
            assert node.level == 0, f"relative import at line {node.lineno}"
            modules.append(node.module)
    assert "torch" in modules
    for m in modules:
        top = m.split(".")[0]
        assert top != "certifiedgpt_amd" and top != "ctypes", m
    assert not any(isinstance(n, ast.Attribute) and n.attr == "cuda" and isinstance(n.value, ast.Name) and n.value.id == "torch"
                   for n in ast.walk(tree)), "llm_laws.py calls into torch.cuda"


def test_the_engine_imports_the_laws_and_not_the_classifier():
    tree = ast.parse(inspect.getsource(llm_engine))
    froms = [(n.level, n.module) for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)]
    assert (1, "llm_laws") in froms and (1, "minigpt4") not in froms
