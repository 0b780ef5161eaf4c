"""CPU: the refusals of prompt_pass="teacher" (auto_reg/t2s_infer.py): the option is score_stream's alone, keeps no cache and
needs the packed pass's head width.  Each is raised with the option named and before the library is touched."""
import pytest
import torch

from test_s1_stream_wide_cpu import _model


def _req():
    return (torch.arange(1, 6), torch.zeros(1024, 5), torch.tensor([3, 4, 5]))


CASES = {
    "decode_stream": (lambda m: m.decode_stream([_req()], prompt_pass="teacher"), "prompt_pass = 'teacher'", {}),
    "refill": (lambda m: m.infer_panel_batch_infer_refill([_req()[0]], None, [_req()[2]], [_req()[1]], prompt_pass="teacher"),
               "prompt_pass = 'teacher'", {}),
    "refill_no_prompts": (lambda m: m.infer_panel_batch_infer_refill([_req()[0]], None, None, [_req()[1]],
                                                                     prompt_pass="teacher"), "prompt_pass = 'teacher'", {}),
    "mxfp8": (lambda m: list(m.score_stream([_req()], [[1, 2]], prompt_pass="teacher", kv_dtype="mxfp8")),
              "prompt_pass = 'teacher'.*kv_dtype = 'mxfp8'", {}),
    "head_width": (lambda m: list(m.score_stream([_req()], [[1, 2]], prompt_pass="teacher")),
                   "prompt_pass = 'teacher' needs a head width of 32, the model's is 64", dict(num_head=8)),
    "keyword": (lambda m: list(m.score_stream([_req()], [[1, 2]], prompt_pass="teacher", early_stop_num=3)),
                "prompt_pass = 'teacher' takes.*early_stop_num", {}),
}


@pytest.fixture(scope="module")
def m():
    return _model()


@pytest.mark.parametrize("name", list(CASES))
def test_teacher_refusals(name, m, monkeypatch):
    from easevoice_trainer_amd.hip import lib as L

    call, match, attrs = CASES[name]
    for k, v in attrs.items():
        monkeypatch.setattr(m, k, v)

    def no_library():
        raise AssertionError("the library was asked for before the refusal")

    monkeypatch.setattr(L, "lib", no_library)
    with pytest.raises(L.EvtError, match=match):
        call(m)
