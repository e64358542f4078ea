"""ops.decode.decode_attn_path: the routing of a decode step's attention is a function of the cache rows and of
MLT_DECODE_SPLIT alone, and no cache as short as those before the split kernels existed is routed to them."""
import pytest

from ml_trainer_amd.ops import decode as DC


@pytest.mark.parametrize("setting", [None, "1", "0"])
def test_decode_attn_path(monkeypatch, setting):
    if setting is None:
        monkeypatch.delenv("MLT_DECODE_SPLIT", raising=False)
    else:
        monkeypatch.setenv("MLT_DECODE_SPLIT", setting)
    assert DC.DECODE_SPLIT_MIN_SMAX > 512
    assert all(DC.decode_attn_path(s) == "single" for s in (1, 128, 256, 511, 512, DC.DECODE_SPLIT_MIN_SMAX - 1))
    want = "single" if setting == "0" else "split"
    assert DC.decode_attn_path(DC.DECODE_SPLIT_MIN_SMAX) == want and DC.decode_attn_path(1 << 15) == want
