"""Line augmentation for the device collator (`BatchCreator(augmenter=LineAugmenter(...))`).

The reference augments on the host, in the dataset, through an opaque callable (`self.augmentations(image=image)`,
common/dataset.py:92-96, 247-254).  Here the host only DRAWS: a handful of integers per line (a small affine transform of the
text line, a smooth displacement field, a tone curve, a noise amplitude and seed).  `pero_augment_stack_lines`
(csrc/augment.hip) applies them while it writes the padded batch, from the same ragged upload `pero_stack_lines` reads.  The
transform keeps every line's width, so image masks, labels and shifts are those of the un-augmented batch.
"""
import math

import numpy as np
import torch

from ..ops import AUGMENT_PARAMS

NOISE_UNIT_STD = math.sqrt(4 * (256 ** 2 - 1) / 12)   # 147.8: the kernel's noise is a sum of four hashed bytes (include/pero_hip.h)
SY, TY, SLOPE, SLANT, NOISE_AMP, SEED_LO, SEED_HI = range(AUGMENT_PARAMS)


def neutral(B, Wt, C, knot_shift=5):
    """The values for which pero_augment_stack_lines writes pero_stack_lines' bytes: (params, knots, lut)."""
    params = torch.zeros((B, AUGMENT_PARAMS), dtype=torch.int32)
    params[:, SY] = 256
    knots = torch.zeros((B, 2, (Wt >> knot_shift) + 2), dtype=torch.int32)
    lut = torch.arange(256, dtype=torch.uint8).repeat(B, C, 1)
    return params, knots, lut


class LineAugmenter:
    """Draws the per-line numbers of pero_augment_stack_lines.  Every magnitude is the half-width of a uniform draw; 0 disables
    that term, and with every magnitude 0 (or p = 0) all lines get the neutral values.

    Geometry (sub-pixel, bilinear, edges replicated):
      max_slope = 0.02         baseline rotation: vertical shift per pixel of x, about the line's centre (0.02 = 1.1 degrees)
      max_slant = 0.15         shear: horizontal shift per pixel of y, about the middle row (3 px at the top of a 40 px line)
      scale_range = 0.08       vertical scale about the middle row, in [1 - 0.08, 1 + 0.08]
      max_translate = 1.5      vertical translation, px
      warp_amplitude_y = 1.0   smooth vertical displacement along the line, px
      warp_amplitude_x = 2.0   smooth horizontal displacement along the line, px.  It must stay below one patch width (the
                               collator's subsampling factor, 8; BatchCreator checks it): labels are attached to patch positions
                               and the transform does not move them, so a pixel may drift inside its neighbourhood of patches but
                               never a whole patch away from its label.  (This is also why there is no horizontal stretch.)
      warp_period = 64         spacing of the coarse knots the displacements are drawn at, px; they are interpolated with a
                               smoothstep to the kernel's knot grid (every 1 << knot_shift = 32 px), so the field is smooth
    Tone (one 256-entry curve per line and channel, built in float, rounded to uint8; the kernel takes it as data):
      gamma = 0.2              v = v ** exp(g), g in [-0.2, 0.2], on v in [0, 1]
      contrast = 0.15          v = (v - 0.5) * (1 + g) + 0.5
      brightness = 0.1         v = v + g
      channel_gain = 0.05      v = v * (1 + g_c), one draw per channel
    Noise:
      noise_sigma = 3.0        per line a standard deviation in [0, 3] grey levels; roughly Gaussian, hashed from the byte's position
                               in the batch and a per-line 64-bit seed
    p = 0.8                    probability that a line is augmented at all
    seed = None                seeds the augmenter's own CPU torch.Generator (None: a fresh random seed).  Nothing is drawn from
                               np.random, so a seeded run collates with the same left paddings and crops with or without it."""

    def __init__(self, max_slope=0.02, max_slant=0.15, scale_range=0.08, max_translate=1.5, warp_amplitude_y=1.0,
                 warp_amplitude_x=2.0, warp_period=64, brightness=0.1, contrast=0.15, gamma=0.2, channel_gain=0.05, noise_sigma=3.0,
                 p=0.8, seed=None, knot_shift=5):
        magnitudes = dict(max_slope=max_slope, max_slant=max_slant, scale_range=scale_range, max_translate=max_translate,
                          warp_amplitude_y=warp_amplitude_y, warp_amplitude_x=warp_amplitude_x, brightness=brightness,
                          contrast=contrast, gamma=gamma, channel_gain=channel_gain, noise_sigma=noise_sigma)
        for name, value in magnitudes.items():
            if not 0 <= value < 1024:
                raise ValueError(f"LineAugmenter: {name} must be in [0, 1024)")
        if scale_range >= 1 or contrast >= 1 or channel_gain >= 1:
            raise ValueError("LineAugmenter: scale_range, contrast and channel_gain must be below 1")
        if not 3 <= knot_shift <= 8 or warp_period < (1 << knot_shift):
            raise ValueError("LineAugmenter: knot_shift must be in [3, 8] and warp_period at least 1 << knot_shift")
        if not 0 <= p <= 1:
            raise ValueError("LineAugmenter: p is a probability")
        for name, value in magnitudes.items():
            setattr(self, name, float(value))
        self.warp_period, self.p, self.knot_shift = int(warp_period), float(p), int(knot_shift)
        self.generator = torch.Generator()
        if seed is None:
            self.generator.seed()
        else:
            self.generator.manual_seed(int(seed))

    def _signed(self, *shape):
        return 2 * torch.rand(shape, generator=self.generator, dtype=torch.float64) - 1

    def _knots(self, B, Wt, amplitude):
        """Coarse knots every warp_period px, uniform in [-amplitude, amplitude] px, smoothstep-interpolated at the columns
        0, K, 2 K, ... of the kernel's grid; 1/256 px.  A convex combination of the draws: it stays inside the amplitude."""
        K, NK = 1 << self.knot_shift, (Wt >> self.knot_shift) + 2
        coarse = self._signed(B, (NK - 1) * K // self.warp_period + 2) * (256 * amplitude)
        pos = torch.arange(NK, dtype=torch.float64) * K / self.warp_period
        j = pos.floor().long()
        f = pos - j
        f = f * f * (3 - 2 * f)
        return torch.round(coarse[:, j] * (1 - f) + coarse[:, j + 1] * f).to(torch.int32)

    def draw(self, widths, H, Wt, C):
        """One draw for the B = len(widths) lines of a (B, H, Wt, C) batch: host tensors params (B, 7) int32, knots (B, 2, NK) int32
        and lut (B, C, 256) uint8.  The number of values taken from the generator depends on (B, Wt, C) only."""
        B = len(widths)
        params, _, identity = neutral(B, Wt, C, self.knot_shift)
        selected = torch.rand(B, generator=self.generator, dtype=torch.float64) < self.p
        g = self._signed(B, 4)
        params[:, SY] = torch.round(256 * (1 + self.scale_range * g[:, 0])).to(torch.int32)
        params[:, TY] = torch.round(256 * self.max_translate * g[:, 1]).to(torch.int32)
        params[:, SLOPE] = torch.round(256 * self.max_slope * g[:, 2]).to(torch.int32)
        params[:, SLANT] = torch.round(256 * self.max_slant * g[:, 3]).to(torch.int32)
        sigma = self.noise_sigma * torch.rand(B, generator=self.generator, dtype=torch.float64)
        params[:, NOISE_AMP] = torch.round(sigma * (65536 / NOISE_UNIT_STD)).to(torch.int32)
        params[:, SEED_LO:] = torch.randint(-2 ** 31, 2 ** 31, (B, 2), generator=self.generator).to(torch.int32)
        params[params[:, NOISE_AMP] == 0, SEED_LO:] = 0       # a seed without noise is not read: keep such a line's row neutral
        knots = torch.stack([self._knots(B, Wt, self.warp_amplitude_y), self._knots(B, Wt, self.warp_amplitude_x)], dim=1)

        t = g.new_tensor(np.arange(256) / 255.0).expand(B, 1, 256)
        tone = self._signed(B, 3, 1, 1)
        v = t ** torch.exp(self.gamma * tone[:, 0])
        v = (v - 0.5) * (1 + self.contrast * tone[:, 1]) + 0.5 + self.brightness * tone[:, 2]
        v = v * (1 + self.channel_gain * self._signed(B, C, 1))
        lut = torch.round(255 * v.clamp(0, 1)).to(torch.uint8)

        off = ~selected
        neutral_params = torch.zeros(AUGMENT_PARAMS, dtype=torch.int32)
        neutral_params[SY] = 256
        params[off] = neutral_params
        knots[off] = 0
        lut[off] = identity[off]
        return params.contiguous(), knots.contiguous(), lut.contiguous()
