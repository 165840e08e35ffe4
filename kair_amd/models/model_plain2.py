"""ModelPlain2 — two-input trainer (the reference's models/model_plain2.py, restated): ModelPlain whose network also
reads data["C"], the per-sample condition (FFDNet: the noise level [B, 1, 1, 1]; the reference trains SRMD with it too).

optimize_parameters runs the fused trainer (the network's step program + pixel loss + fused Adam / EMA, one HIP graph
per step) with C as the step's extra input: a replay reads the C of its own batch.
"""
from .model_plain import ModelPlain


class ModelPlain2(ModelPlain):
    def feed_data(self, data, need_H=True):
        self.L = data["L"].to(self.device, non_blocking=True)
        self.C = data["C"].to(self.device, non_blocking=True)
        if need_H:
            self.H = data["H"].to(self.device, non_blocking=True)

    def _step_cond(self):
        """The network's second input for the fused, graph-captured step."""
        return (self.C,)

    def netG_forward(self):
        self.E = self.netG(self.L, self.C)
