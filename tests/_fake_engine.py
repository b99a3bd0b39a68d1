"""binding.Engine's surface as diffusion.py / selection.py / verified.py use it, on the CPU, with every numeric property a knob.

Logits are an exact integer function of (row, position, class, t) — no token values, no random generator — plus, per precision, an
injected error of exactly `noise * max |logit|` with a fixed sign pattern, so whatever is recorded from a run (tools/make_selection_golden.py)
depends on no random stream and on no torch build."""
import torch


class FakeEngine:
    fast_noise = 0.0
    mixed_noise = 0.0
    hybrid_noise = 1.0            # (far outside unless a test sets it)
    split_noise = 0.0             # the split engine's error against the fp32-MFMA probe engine
    mixed_available = True
    nonfinite = ()                # precisions whose logits carry an inf
    refuse = {}                   # precision -> text of the RuntimeError its constructor raises
    built = []                    # (precision, max_batch) in build order
    live = peak = 0               # engines built and not closed, and the largest value that count took
    double_closes = 0

    @classmethod
    def reset(cls):
        cls.fast_noise, cls.mixed_noise, cls.hybrid_noise, cls.split_noise, cls.mixed_available = 0.0, 0.0, 1.0, 0.0, True
        cls.nonfinite, cls.refuse, cls.built = (), {}, []
        cls.live = cls.peak = cls.double_closes = 0

    def __init__(self, *, n_category, n_bin=32, max_elem=25, n_attr=5, n_step=100, precision="exact", max_batch=512,
                 q_type="constrained", **_k):
        self.q_type = q_type
        self.S, self.C, self.T = max_elem * n_attr, n_category + 4 * n_bin + 2, n_step
        self.n_attr, self.n_bin, self.n_category = n_attr, n_bin, n_category
        self.pad_id, self.mask_id = self.C - 2, self.C - 1
        self.max_batch, self.batch_round, self.precision = max_batch, 256, precision
        self.device = torch.device("cpu")
        if precision in FakeEngine.refuse:
            raise RuntimeError(FakeEngine.refuse[precision])
        if precision in ("mixed", "hybrid") and not FakeEngine.mixed_available:
            raise RuntimeError("ldm_create: precision mixed: only the reference backbone's geometry ...")
        FakeEngine.built.append((precision, max_batch))
        self.closed = False
        FakeEngine.live += 1
        FakeEngine.peak = max(FakeEngine.peak, FakeEngine.live)

    def load_state_dict(self, sd):
        pass

    def _tok(self, t):
        return torch.as_tensor(t).to(torch.int32).contiguous()

    def denoise_logits(self, tokens, t):
        tokens = self._tok(tokens)
        assert tokens.shape[0] <= self.max_batch, f"batch {tokens.shape[0]} outside [1, max_batch = {self.max_batch}]"
        r, p, c = torch.meshgrid(torch.arange(tokens.shape[0]), torch.arange(self.S), torch.arange(self.C), indexing="ij")
        base = ((7 * r + 13 * p + 29 * c + 31 * int(t)) % 201 - 100).float()
        noise = {"fast": FakeEngine.fast_noise, "mixed": FakeEngine.mixed_noise, "hybrid": FakeEngine.hybrid_noise,
                 "split": FakeEngine.split_noise}.get(self.precision, 0.0)
        if noise:
            base = base + noise * base.abs().max() * (1 - 2 * ((r + p + c) % 2)).float()
        if self.precision in FakeEngine.nonfinite:
            base[0, 0, 0] = float("inf")
        return base

    def sample_loop(self, tokens, t_model, t_post, cfg, cond=None, seed=0, first_layout=0, intermediates=False, use_graph=True,
                    lc_keep=None, relation=None):
        tokens = self._tok(tokens)
        inter = torch.stack([tokens.clone() for _ in t_model]) if intermediates else None
        return tokens, inter

    def set_tie_report(self, *a, **k):
        pass

    def describe(self):
        return {"precision": self.precision}

    def close(self):
        if self.closed:
            FakeEngine.double_closes += 1
            return
        self.closed = True
        FakeEngine.live -= 1
