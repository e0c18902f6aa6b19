"""The fixture tests/test_input_cpu.py and tests/test_gpu_input.py share: a [7, 20, 28, 3] uint8 source (non-square; a row is 84
bytes, no multiple of 16), a batch of five with a repeated sample, and the boxes of the window and bilinear cases."""
import torch

IDX = [3, 0, 6, 3, 1]
FLIP = [1, 0, 1, 0, 0]
H, W = 20, 28

# window mode: (S_h, S_w, boxes (top, left, h, w) per sample or None); h, w are not read there
WINDOW_CASES = {
    "16x16 at odd left": (16, 16, [(0, 1, 16, 16), (2, 5, 16, 16), (4, 11, 16, 16), (3, 1, 16, 16), (1, 5, 16, 16)]),
    "13x13": (13, 13, [(7, 15, 13, 13), (0, 0, 13, 13), (5, 3, 13, 13), (2, 14, 13, 13), (6, 7, 13, 13)]),
    "full": (20, 28, [(0, 0, 20, 28)] * 5),
    "centred 16x16": (16, 16, None),
    "centred 13x13": (13, 13, None),
}

_GENERAL = [(3, 5, 13, 21), (0, 0, 20, 28), (7, 9, 11, 13), (1, 2, 17, 19), (3, 5, 13, 21)]
# bilinear mode: (S, boxes, dyadic): dyadic weights make every product and sum exact in float32 and float64
BILINEAR_CASES = {
    "general onto 16": (16, _GENERAL, False),
    "general onto 17": (17, _GENERAL, False),
    "8x8 onto 16 (dyadic)": (16, [(2, 4, 8, 8)] * 5, True),
}
TIE_EPS = 1e-4          # |v - (k + 1/2)| below this, v not a half-integer: the level may differ by one
TIE_SHARE = 0.01        # at most this share of a case's values may be such


def source():
    return torch.randint(0, 256, (7, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(20))
