"""The e4m3 KV cache option on the CPU side: the C ABI refuses a bad format before it looks at the context, the binding lists the new entry
points, and the command lines parse --fp8_kv without changing what --compare_fp8 switches when it is not given."""
import ctypes

import pytest


def test_alloc_ex_checks_the_format_before_the_context():
    from callireader_amd import _binding as B
    out = ctypes.c_void_p()
    assert B.lib.cr_kv_alloc_ex(None, 1, 16, 7, ctypes.byref(out)) == -1          # CR_ERR_ARG
    msg = B.lib.cr_last_error().decode()
    assert 'format' in msg and '7' in msg, msg
    assert B.lib.cr_kv_alloc_ex(None, 1, 16, B.CR_KV_E4M3, ctypes.byref(out)) == -1
    msg = B.lib.cr_last_error().decode()
    assert 'context' in msg and 'format' not in msg, msg
    assert B.lib.cr_kv_alloc_ex(None, 1, 16, B.CR_KV_BF16, ctypes.byref(out)) == -1
    assert 'context' in B.lib.cr_last_error().decode()
    assert B.lib.cr_kv_format(None) < 0


def test_binding_lists_the_e4m3_entry_points():
    from callireader_amd import _binding as B
    for name in ('cr_kv_alloc_ex', 'cr_kv_format', 'cr_kv_read_e4m3', 'cr_op_decode_attention_e4m3'):
        assert name in B.SIGNATURES
        assert hasattr(B.lib, name)
    assert B.ABI_VERSION == 13 and B.lib.cr_abi_version() == 13
    assert (B.CR_KV_BF16, B.CR_KV_E4M3) == (0, 1)


def test_op_decode_attention_e4m3_refuses_bad_arguments_without_a_gpu():
    from callireader_amd import _binding as B
    assert B.lib.cr_op_decode_attention_e4m3(0, None, None, None, None, None, 16, None, None, 1, 1, 1.0, None, None, None) == -1
    assert b'cr_op_decode_attention_e4m3' in B.lib.cr_last_error()


def test_kv_dtype_names():
    from callireader_amd.engine import kv_format
    assert kv_format('bf16') == 0 and kv_format('e4m3') == 1
    for bad in ('fp8', 'float8_e4m3fn', None, 1):
        with pytest.raises(ValueError):
            kv_format(bad)


def test_inference_parses_fp8_kv():
    from callireader_amd import inference
    p = inference.build_parser()
    assert p.parse_args(['--tgt', 'x']).fp8_kv is False
    assert p.parse_args(['--tgt', 'x', '--fp8_kv']).fp8_kv is True


def test_evaluate_compare_fp8_switches():
    from callireader_amd import evaluate
    p = evaluate.build_parser()
    sw = lambda *a: evaluate.fp8_switches(p.parse_args(list(a)))      # noqa: E731
    assert p.parse_args([]).fp8_kv is False
    # without --fp8_kv: exactly the switches (and the report keys) --compare_fp8 always had
    assert sw('--compare_fp8') == {'fp8_mfma': 1, 'fp8_decode': True}
    assert sw('--compare_fp8', '--fp8_decode') == {'fp8_mfma': 0, 'fp8_decode': True}
    assert sw('--compare_fp8', '--fp8_mfma', '2') == {'fp8_mfma': 2, 'fp8_decode': False}
    assert sw() == {'fp8_mfma': 0, 'fp8_decode': False}
    # with it, it joins the fp8 arm
    assert sw('--compare_fp8', '--fp8_kv') == {'fp8_mfma': 1, 'fp8_decode': True, 'fp8_kv': True}
    assert sw('--compare_fp8', '--fp8_decode', '--fp8_kv') == {'fp8_mfma': 0, 'fp8_decode': True, 'fp8_kv': True}
    assert sw('--fp8_kv') == {'fp8_mfma': 0, 'fp8_decode': False, 'fp8_kv': True}
