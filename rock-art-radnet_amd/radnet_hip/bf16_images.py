"""The bf16 weight images of an engine (precision "bf16" / "bf16-mixed" / "bf16-train"): one owner for the forward image of a layer,
its dgrad image, and per optimizer arena the two registries Adam hands to the library.

An image is created by a cast launch on the lane that is current at that moment (the engine's `ctx` switches inside lane()) and is
rewritten in place from then on, so compiled programs and recorded hipGraphs keep their pointers."""
import collections

import torch

from . import lib as L

FwdImage = collections.namedtuple("FwdImage", "wt ldk conv n")        # bf16 copy [n][ldk] of conv.weight (ldk = K rounded up to 32)
DgradImage = collections.namedtuple("DgradImage", "wd ldkd conv n")   # dgrad image [cin][ldkd] of conv.weight (bf16-train)
AdamLayers = collections.namedtuple("AdamLayers", "array count")      # radnet_adam_bf16[]: the forward images Adam rewrites for an arena


class DgradRegistry:
    """radnet_bf16_dgrad_image[]: the dgrad images of one arena's layers, rewritten by one cast launch behind its Adam."""
    CAP = 16

    def __init__(self):
        self.array, self.count = (L.Bf16DgradImage * self.CAP)(), 0


class Bf16Images:
    def __init__(self, engine):
        self.eng = engine
        self.fwd = {}              # fp32 weight pointer -> FwdImage
        self.dgrad = {}            # fp32 weight pointer -> DgradImage
        self.adam = {}             # id(arena) -> AdamLayers
        self.dgrad_arena = {}      # id(arena) -> DgradRegistry
        self._layers = None

    def layer(self, wptr):
        """The conv layer whose fp32 weights live at `wptr` (what a descriptor's `w` holds)."""
        if self._layers is None:
            self._layers = {c.weight.data_ptr(): c for c in self.eng.convs.values() if c.weight is not None}
        return self._layers[wptr]

    def forward_image(self, wptr):
        return self.weights(self.layer(wptr))

    def dgrad_image(self, wptr):
        return self.dgrad_weights(self.layer(wptr))

    def weights(self, c):
        """bf16 copy [N][ldk] of conv `c`'s weights (N = the descriptor's output columns, ldk = K rounded up to 32), made on first
        use; refresh() rewrites it in place whenever the weights change, so compiled programs and hipGraphs keep their pointers."""
        ent = self.fwd.get(c.weight.data_ptr())
        if ent is None:
            k = c.kh * c.kh * c.cin
            n = c.ldw if c.name == "rpn_heads" else c.cout
            ldk = (k + 31) // 32 * 32
            wt = torch.empty(n, ldk, dtype=torch.int16, device=self.eng.dev)
            ent = FwdImage(wt, ldk, c, n)
            self.fwd[c.weight.data_ptr()] = ent
            self.eng.ctx.call("radnet_weights_to_bf16", c.weight, k, n, c.ldw, wt, ldk)
        return ent

    def refresh(self):
        for im in self.fwd.values():
            c = im.conv
            self.eng.ctx.call("radnet_weights_to_bf16", c.weight, c.kh * c.kh * c.cin, im.n, c.ldw, im.wt, im.ldk)
        for im in self.dgrad.values():
            c = im.conv
            self.eng.ctx.call("radnet_weights_to_bf16_dgrad", c.weight, c.kh * c.kh, c.cin, im.n, c.ldw, im.wd, im.ldkd)

    def dgrad_weights(self, c):
        """bf16-train: the dgrad image [cin][ldkd] of conv `c` (radnet_weights_to_bf16_dgrad: element tap * n8 + j of row i is
        bf16(w[(tap, i)][j]), n8 = N rounded up to 8, ldkd = taps * n8 rounded up to 32), made on first use and entered into its
        arena's registry; refresh() and the engine's adam() rewrite it in place, so compiled programs and hipGraphs keep their pointers."""
        ent = self.dgrad.get(c.weight.data_ptr())
        if ent is None:
            taps = c.kh * c.kh
            n = c.ldw if c.name == "rpn_heads" else c.cout
            ldkd = (taps * ((n + 7) // 8 * 8) + 31) // 32 * 32
            wd = torch.empty(c.cin, ldkd, dtype=torch.int16, device=self.eng.dev)
            ent = DgradImage(wd, ldkd, c, n)
            self.dgrad[c.weight.data_ptr()] = ent
            self.eng.ctx.call("radnet_weights_to_bf16_dgrad", c.weight, taps, c.cin, n, c.ldw, wd, ldkd)
            for arena in (self.eng.rpn_arena, self.eng.head_arena):
                lo = arena.p.data_ptr()
                if lo <= c.weight.data_ptr() < lo + 4 * arena.n:
                    reg = self.dgrad_arena.setdefault(id(arena), DgradRegistry())
                    if reg.count >= reg.CAP:
                        raise L.RadnetError("engine: more than 16 dgrad images in one optimizer arena")
                    r = reg.array[reg.count]
                    r.off, r.taps, r.c, r.n, r.ldw, r.wd, r.ldkd = (c.weight.data_ptr() - lo) // 4, taps, c.cin, n, c.ldw, wd.data_ptr(), ldkd
                    reg.count += 1
        return ent

    def adam_layers(self, arena):
        """bf16-mixed: AdamLayers(radnet_adam_bf16[], n) -- the registry of the bf16 images whose fp32 masters live in `arena` (rpn_conv1
        and rpn_heads in the RPN arena, the ten stage-5 convs in the head arena), made on first use together with any image not made yet.
        Adam #1 and the RPN forwards run on the main lane, Adam #2 and the classifier forward on the head lane: each image is written
        and read on one lane.  The frozen base's images are written once per weight load (set_weights)."""
        ent = self.adam.get(id(arena))
        if ent is None:
            lo, hi = arena.p.data_ptr(), arena.p.data_ptr() + 4 * arena.n
            rows = []
            for c in self.eng.convs.values():
                if c.weight is not None and c.cin % 8 == 0 and lo <= c.weight.data_ptr() < hi:
                    im = self.weights(c)
                    rows.append(((c.weight.data_ptr() - lo) // 4, c.kh * c.kh * c.cin, im.n, c.ldw, im.wt.data_ptr(), im.ldk))
            arr = (L.AdamBf16 * max(len(rows), 1))()
            for k, (off, kk, n, ldw, wt, ldk) in enumerate(rows):
                arr[k].off, arr[k].k, arr[k].n, arr[k].ldw, arr[k].wt, arr[k].ldk = off, kk, n, ldw, wt, ldk
            ent = AdamLayers(arr, len(rows))
            self.adam[id(arena)] = ent
        return ent
