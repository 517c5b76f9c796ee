"""No GPU: the numpy model of one wavefront of ``csrc/stft_block.hip`` (``tools/check_stft_block_lds.py``) -- the radix-4
index arithmetic and the real-transform split / merge passes reproduce ``np.fft``, and no LDS instruction of the
exchanges has a bank conflict by the gfx950 rules for 8-byte accesses."""
import os
import re

from conftest import ROOT
from tools import check_stft_block_lds as model


def test_wave_model_matches_numpy_fft_without_bank_conflicts():
    err_f, err_i, worst = model.main()
    assert err_f < 1e-11 and err_i < 1e-12
    assert worst and all(extra == 0 for extra in worst.values()), worst


def test_model_and_kernel_share_the_layout_constants():
    src = open(os.path.join(ROOT, "nested-u-net-based-real-time-speech-enhancement-mobile-app_amd", "csrc", "stft_block.hip")).read()
    assert int(re.search(r"constexpr int kImage = (\d+);", src).group(1)) == model.IMAGE
    assert "return k ^ (((k >> 4) & 1) << 1) ^ ((k >> 5) & 1);" in src          # nat()
    assert "return k ^ ((k >> 4) & 1);" in src                                    # spec()
    for expr in ("80 * k0 + l0 + 16 * a", "80 * k0 + 20 * k1 + l00 + 4 * a", "80 * k0 + 20 * k1 + 4 * l00 + (q ^ l00)",
                 "80 * k0 + 20 * k1 + 4 * a + (l00 ^ a)"):
        assert expr in src, expr
