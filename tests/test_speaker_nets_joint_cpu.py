"""Argument checks of the entry points that serve several models in one launch (crk_adam_step_multi,
crk_nets_prepare_models): CRK_ERR_ARG comes back before anything is launched, so these run without a GPU.  (That header,
binding and library agree on the new argument lists is tests/test_oracle_cpu.py's check over every declared function.)"""
import ctypes

from crank_amd import _lib

CRK_ERR_ARG = 1


def _block(n=16, **over):
    fake = 0x1000  # never dereferenced: every call below is refused by the argument checks
    f = dict(params=fake, grads=fake + 64, exp_avg=fake + 128, exp_avg_sq=fake + 192, n=n, lr_dev=fake + 256, step_dev=fake + 320)
    f.update(over)
    return f


def _call(blocks, n_blocks=None):
    rec = (_lib.AdamBlock * max(len(blocks), 1))()
    for r, f in zip(rec, blocks):
        for k, v in f.items():
            setattr(r, k, v)
    return _lib.lib().crk_adam_step_multi(len(blocks) if n_blocks is None else n_blocks, rec, 0.9, 0.999, 1e-8, 1, None)


def test_adam_step_multi_refuses_bad_arguments_before_any_launch():
    L = _lib.lib()
    assert L.crk_adam_step_multi(1, None, 0.9, 0.999, 1e-8, 1, None) == CRK_ERR_ARG  # no record
    assert _call([]) == CRK_ERR_ARG and _call([_block()], n_blocks=-1) == CRK_ERR_ARG  # no blocks
    assert _call([_block(step_dev=0x2000 + 8 * i) for i in range(_lib.ADAM_MAX_BLOCKS + 1)]) == CRK_ERR_ARG  # more than the record holds
    assert _call([_block(), _block(n=-1, step_dev=0x3000)]) == CRK_ERR_ARG  # negative count
    for field in ("params", "grads", "exp_avg", "exp_avg_sq", "lr_dev", "step_dev"):  # a null pointer in a block
        assert _call([_block(), _block(**dict({"step_dev": 0x3000}, **{field: None}))]) == CRK_ERR_ARG, field
    assert _call([_block(), _block()]) == CRK_ERR_ARG  # one step count named twice: it would advance twice


def test_record_sizes_match_the_header():
    header = open(__file__.replace("tests/test_speaker_nets_joint_cpu.py", "include/crank_hip.h")).read()
    assert f"#define CRK_ADAM_MAX_BLOCKS {_lib.ADAM_MAX_BLOCKS}\n" in header
    assert ctypes.sizeof(_lib.AdamBlock) == 7 * 8  # four pointers, a long long, two pointers


def test_nets_prepare_models_refuses_bad_arguments_before_any_launch():
    L = _lib.lib()
    one = (ctypes.c_void_p * 1)(0x1000)
    ver = (ctypes.c_ulonglong * 1)(1)
    five = (ctypes.c_void_p * 5)(*[0x2000 + 8 * i for i in range(5)])
    assert L.crk_nets_prepare_models(-1, one, one, ver, 0, None, None) == CRK_ERR_ARG
    assert L.crk_nets_prepare_models(1, None, one, ver, 0, None, None) == CRK_ERR_ARG
    assert L.crk_nets_prepare_models(1, one, None, ver, 0, None, None) == CRK_ERR_ARG
    assert L.crk_nets_prepare_models(1, one, one, None, 0, None, None) == CRK_ERR_ARG
    assert L.crk_nets_prepare_models(0, None, None, None, 5, five, None) == CRK_ERR_ARG  # more step counts than the record holds
    assert L.crk_nets_prepare_models(0, None, None, None, -1, five, None) == CRK_ERR_ARG
    assert L.crk_nets_prepare_models(0, None, None, None, 2, None, None) == CRK_ERR_ARG
    assert L.crk_nets_prepare_models(0, None, None, None, 2, (ctypes.c_void_p * 2)(0x2000, None), None) == CRK_ERR_ARG  # a null count
    assert L.crk_nets_prepare_models(1, (ctypes.c_void_p * 1)(None), one, ver, 0, None, None) == CRK_ERR_ARG  # a null net
    assert L.crk_nets_wnorm_bwd(1, (ctypes.c_void_p * 1)(None), None) == CRK_ERR_ARG
