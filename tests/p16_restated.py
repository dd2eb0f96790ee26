"""Restatement of the library's two-plane ("P16") split of an fp32 value (csrc/device_utils.h split_f16, csrc/gemm_p16.hip to_p16 /
from_p16), the yardstick of tests/test_p16_abi.py (hand-worked values) and tests/test_hip_kernels_p16.py (against the device).
Written from the formula, every step in fp32 with round to nearest even, on the device of its input:

  xc = clamp(x, -65504, 65504);  h = fp16(xc);  l = fp16((xc - h) * lscale);  value = h + l / lscale

xc - h is exact (|xc - h| <= ulp(h) / 2), lscale is a power of two (2048 for GEMM operands, 1 for the q|k|v image the attention
kernel reads), so the only roundings are the two conversions to fp16."""
import torch

F16_MAX = 65504.0


def split(x, lscale=2048.0):
    """(h, l) as fp16 tensors"""
    xc = x.float().clamp(-F16_MAX, F16_MAX)
    h = xc.to(torch.float16)
    l = ((xc - h.float()) * lscale).to(torch.float16)
    return h, l


def p16(x, lscale=2048.0):
    """the fp32 value a P16 image holds for x"""
    h, l = split(x, lscale)
    return h.float() + l.float() / lscale


def heads(x):
    """the head plane alone, as fp32: what MODE 1 (fast16) multiplies"""
    return x.float().clamp(-F16_MAX, F16_MAX).to(torch.float16).float()


def image_bits(x, lscale=2048.0):
    """x [M, C] (C % 32 == 0) -> the image as stored, int16 [M, 2 * C]: per 32-channel group 32 heads then 32 residuals"""
    M, C = x.shape
    h, l = split(x, lscale)
    img = torch.stack([h.view(M, C // 32, 32), l.view(M, C // 32, 32)], dim=2)
    return img.reshape(M, 2 * C).view(torch.int16)
