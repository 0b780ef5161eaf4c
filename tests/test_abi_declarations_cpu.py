"""The Python/C boundary without a GPU: the header parser of hip/lib.py on a synthetic header, the package's evt_* call sites
counted against include/evt.h with `ast`, what a typed declaration refuses before a launch, and the refusals of the one
length check of the ragged launches."""
import ast
import ctypes as C
import os
import re

import pytest
import torch

from easevoice_trainer_amd.hip import lib as L

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(HERE, "..", "easevoice_trainer_amd")

SYNTHETIC = """
#ifndef T_H
#define T_H
#define T_MACRO(a, b) \\
    t_not_a_function(a, b);
/* int t_in_block_comment(int32_t a);
 * int t_in_block_comment_too(void); */
// int t_behind_slashes(int32_t a);
typedef struct t_params { int32_t a, b; float c; } t_params;
const char* t_name(void);
void t_switch(int32_t enable);   // int t_behind_code(void);
int32_t t_code(const t_params* p);
int64_t t_floats(int32_t n, int64_t m);
int t_launch(const float* const* p,
             uint32_t seed, float eps,   /* int t_inside(void); */
             void* stream);
#endif
"""


def test_prototypes_of_a_synthetic_header():
    protos = L.prototypes(SYNTHETIC)
    assert protos == {
        "t_name": (C.c_char_p, []),
        "t_switch": (None, [C.c_int32]),
        "t_code": (C.c_int32, [C.c_void_p]),
        "t_floats": (C.c_int64, [C.c_int32, C.c_int64]),
        "t_launch": (C.c_int, [C.c_void_p, C.c_uint32, C.c_float, C.c_void_p]),
    }
    for decl, param in (("int t_bad(int32_t n, double x);", "double x"), ("int t_bad(size_t n);", "size_t n"),
                        ("int t_bad(void* q, evt_conv_params p);", "evt_conv_params p")):
        with pytest.raises(L.EvtError, match=f"t_bad.*{param}"):
            L.prototypes(SYNTHETIC + decl)
    with pytest.raises(L.EvtError, match="t_bad.*double"):
        L.prototypes("double t_bad(void);")
    with pytest.raises(L.EvtError, match="t_bad"):
        L.prototypes("float* t_bad(void);")


def _header_counts():
    """{name: parameters} of include/evt.h by comma count, independent of the library's parser"""
    hdr = open(os.path.join(HERE, "..", "include", "evt.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    return {m.group(1): 0 if m.group(2).strip() == "void" else m.group(2).count(",") + 1
            for m in re.finditer(r"\b(evt_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", hdr)}


def _evt_calls(tree):
    """(name, positional count or None for a call with *args, line) of every evt_* call of a module: `<expr>.evt_x(...)`,
    and `fn(...)` where `fn = <expr>.evt_x` is the only binding of `fn` in the same function"""
    found = []
    scopes = [tree] + [n for n in ast.walk(tree) if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef, ast.Lambda))]
    for scope in scopes:
        body = []          # the nodes of this scope alone: nested functions are scopes of their own
        todo = list(ast.iter_child_nodes(scope))
        while todo:
            n = todo.pop()
            body.append(n)
            if not isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef, ast.Lambda)):
                todo.extend(ast.iter_child_nodes(n))
        bound, stores = {}, {}
        for n in body:
            if isinstance(n, ast.Name) and isinstance(n.ctx, ast.Store):
                stores[n.id] = stores.get(n.id, 0) + 1
            if (isinstance(n, ast.Assign) and len(n.targets) == 1 and isinstance(n.targets[0], ast.Name)
                    and isinstance(n.value, ast.Attribute) and n.value.attr.startswith("evt_")):
                bound[n.targets[0].id] = n.value.attr
        for n in body:
            if not isinstance(n, ast.Call):
                continue
            if isinstance(n.func, ast.Attribute) and n.func.attr.startswith("evt_"):
                name = n.func.attr
            elif isinstance(n.func, ast.Name) and n.func.id in bound and stores[n.func.id] == 1:
                name = bound[n.func.id]
            else:
                continue
            assert not n.keywords, f"line {n.lineno}: {name} called with keywords"
            starred = any(isinstance(a, ast.Starred) for a in n.args)
            found.append((name, None if starred else len(n.args), n.lineno))
    return found


# the calls that pass *args: their count is not visible to this test (ctypes still checks it at the call).  The two calls
# of auto_reg/t2s_infer.py that choose their entry point by name (getattr) are out of its reach as well.
STARRED_CALLS = ["module/losses.py: evt_masked_kl_fwd", "module/losses.py: evt_masked_kl_bwd"]


def test_call_sites_pass_what_the_header_declares():
    """every evt_* call of the package passes as many positional arguments as include/evt.h declares parameters"""
    counts = _header_counts()
    assert len(counts) > 100
    wrong, starred, seen = [], [], 0
    for root, _, files in sorted(os.walk(PKG)):
        for f in sorted(files):
            if not f.endswith(".py"):
                continue
            path = os.path.join(root, f)
            rel = os.path.relpath(path, PKG).replace(os.sep, "/")
            for name, n, line in _evt_calls(ast.parse(open(path).read())):
                seen += 1
                if name not in counts:
                    wrong.append(f"{rel}:{line}: {name} is not declared in evt.h")
                elif n is None:
                    starred.append(f"{rel}: {name}")
                elif n != counts[name]:
                    wrong.append(f"{rel}:{line}: {name} takes {counts[name]} arguments, the call passes {n}")
    assert seen > 100, "the walk found too few call sites to be looking at the package"
    assert not wrong, "\n".join(wrong)
    assert sorted(starred) == sorted(STARRED_CALLS)


def test_typed_declarations_refuse_before_a_launch():
    """evt_hubert_front_rows(int32_t dtype, x, lens, int32_t nseq, int32_t N, weight, gamma, beta, float eps, out, ws,
    int64_t ws_floats, stream) with NULL pointers: ctypes refuses a wrong kind or count, the library the NULL pointers"""
    fn = L.lib().evt_hubert_front_rows
    with pytest.raises(C.ArgumentError):
        fn(L.DT_F32, None, None, 1.0, 100, None, None, None, 1e-5, None, None, 0, None)
    with pytest.raises(C.ArgumentError):
        fn(L.DT_F32, None, None, C.c_int64(1), 100, None, None, None, 1e-5, None, None, 0, None)
    with pytest.raises(TypeError):
        fn(L.DT_F32, None, None, 1, 100, None, None, None, 1e-5, None, None, 0)
    assert fn(L.DT_F32, None, None, 1, 100, None, None, None, 1, None, None, 0, None) == L.EVT_EINVAL


def _lens_cases(nseq):
    """(what is wrong, lens, mul, x requires grad)"""
    good = torch.full((nseq,), 4, dtype=torch.int32)
    return [("int64 lens", good.long(), 1, False),
            ("3 entries", torch.full((nseq + 1,), 4, dtype=torch.int32), 1, False),
            ("a stride-2 view", torch.full((2 * nseq,), 4, dtype=torch.int32)[::2], 1, False),
            ("mul = 0", good, 0, False),
            ("x requires grad", good, 1, True)]


@pytest.mark.parametrize("op", ["mask_tail", "mish_rows", "hubert_front_rows", "resample_pack", "resample_pack_rows"])
def test_check_lens_refusals(op):
    """refusing cases only, on CPU tensors: nothing reaches a kernel.  resample_pack takes rows [nseq, L]: at [2, 16, 8] its
    own shape check refuses first, so the same cases also run at [2, 16], where they reach check_lens"""
    from easevoice_trainer_amd.hip import audio, conv, enc, feat

    assert torch.is_grad_enabled()
    name = "resample_pack" if op == "resample_pack_rows" else op
    shape = {"hubert_front_rows": (2, 400), "resample_pack_rows": (2, 16)}.get(op, (2, 16, 8))
    for wrong, lens, mul, grad in _lens_cases(2):
        x = torch.zeros(shape, requires_grad=grad)
        if wrong == "a stride-2 view":
            assert not lens.is_contiguous() and lens.numel() == 2
        if mul != 1 and op in ("mish_rows", "hubert_front_rows"):
            continue                                   # no mul to give
        with pytest.raises(L.EvtError) as err:
            if op == "mask_tail":
                conv.mask_tail(x, lens, mul)
            elif op == "mish_rows":
                enc.mish_rows(x, lens)
            elif op == "hubert_front_rows":
                w = torch.zeros(512, 10)
                feat.hubert_front_rows(x, lens, w, torch.ones(512), torch.zeros(512), 1e-5, torch.float32)
            else:
                audio.resample_pack(x, [4, 4], mul, 32000, 32000, "int16", lens_dev=lens)
        assert str(err.value).startswith(name), f"{op}, {wrong}: {err.value}"
