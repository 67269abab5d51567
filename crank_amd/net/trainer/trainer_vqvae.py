"""VQ-VAE trainer: per step a G update (reconstruction + commitment + STFT +
speaker-adversarial terms), a SPKRADV update and a speaker-classifier C update, with
the optional cyclic variant.  Follows crank/net/trainer/trainer_vqvae.py (train :58-68,
forward_vqvae :121-137, forward_cycle :139-161, forward_spkradv :163-184,
forward_spkrclassifier :186-198, step_model :200-208, loss algebra :210-357).

Deviations that do not change the numbers: masked means are taken by the masked loss
kernel instead of masked_select + mean (no compaction, no hidden host sync), and
networks whose parameter gradients the reference computes only to discard (quirk Q7)
skip their weight-gradient kernels.
"""

import torch

from ... import parallel
from ...config import cfg
from .basetrainer import BaseTrainer
from .utils import clip_grad_norm as flat_clip_grad_norm


def _one_like(t):
    """The cached root gradient (crank_amd.ops.one_like where the tensor lives on the GPU: the loss-total op recognises it)."""
    if t.is_cuda:
        from ... import ops
        return ops.one_like(t)
    key = (t.device, t.dtype, tuple(t.shape))
    if key not in _ONES:
        _ONES[key] = torch.ones_like(t)
    return _ONES[key]


_ONES = {}


def _scaled(w, t):
    """w * t without a launch when w is exactly 1 (the default alpha["ce"])."""
    return t if float(w) == 1.0 else w * t


class VQVAETrainer(BaseTrainer):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.cycle_flag = False
        self._check_cycle_start()

    def check_custom_start(self):
        self._check_cycle_start()

    # ------------------------------------------------------------------ step
    def train(self, batch, phase="train"):
        self._cond_cache = None  # conditioning tensors are shared by the sub-updates of ONE step only
        self._label_cache = None  # (a captured step must contain the launches that build them: never carried across steps)
        self._open_arena()  # the loss ops' result scalars of this step side by side: one copy to the host, no stacking launch
        loss = self._get_loss_dict(batch)
        # Data parallel: the generator's gradient all-reduce (5.2 MB, the largest message of the step) is started when its
        # backward is done and completed just before its Adam step; the speaker classifier's whole update - which reads
        # neither the generator's parameters nor its gradients (trainer_vqvae.py:186-198) - is enqueued in between and
        # runs in the shadow of the collective.  Same values as the reference order (G, SPKRADV, C): the three updates
        # only meet through the generator's NEW parameters, which the speaker-adversarial update still sees.
        self._G_tail = None
        self._defer_G_tail = (phase == "train" and parallel.is_dist() and self.conf["use_spkr_classifier"]
                              and self._G_step_is_last_of_main_update())
        # ... and the classifier's own gradient message (0.6 MB) waits for the speaker-adversarial net's (0.16 MB): the two
        # travel at ONE point of the step (one collective boundary instead of two), followed by both Adam steps.  Nothing
        # reads the classifier's new parameters before the next step.
        self._C_tail = None
        self._defer_C_tail = self._defer_G_tail and self.conf["use_spkradv_training"]
        # Single process: the same independence lets the classifier's update run on a second stream next to the rest of
        # the step (its kernels are small and latency bound - 8 layers of 64 channels - and fill the compute units the
        # step's dependent launches leave idle).  Forked here, joined before the loss values are collected; inside a
        # captured step the fork and the join become edges of the graph.  Same values: nothing is shared but the batch.
        # That is config.cfg.overlap_c = 1 / 2.  The default, 3, keeps the classifier's update in line and gives it and the
        # speaker-adversarial net's update one set of maintenance launches instead (update_speaker_nets): the second stream
        # hid 9 us of the classifier's update, the shared launches take 33 us of kernel time off the stream.
        side = self._classifier_stream(batch, phase)
        late = cfg.overlap_c == 2

        def fork_classifier(loss):
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                return self.forward_spkrclassifier(batch, loss, phase=phase)

        if side is not None and not late:
            loss = fork_classifier(loss)
        loss = self._main_update(batch, loss, phase)
        if side is not None and late:
            loss = fork_classifier(loss)
        if self._G_tail is not None:
            self._defer_G_tail = False
            loss = self.forward_spkrclassifier(batch, loss, phase=phase)
            tail, self._G_tail = self._G_tail, None
            tail()
            loss = self.forward_spkradv(batch, loss, phase=phase)
        else:
            self._defer_G_tail = False
            if side is None and self._speaker_updates_joinable(batch, phase):
                loss = self.update_speaker_nets(batch, loss, phase=phase)
            else:
                loss = self.forward_spkradv(batch, loss, phase=phase)
                if side is None:
                    loss = self.forward_spkrclassifier(batch, loss, phase=phase)
        if self._C_tail is not None:  # (nobody took the classifier's message along: its own reduce and step)
            tail, self._C_tail = self._C_tail, None
            tail()
        self._defer_C_tail = False
        if side is not None:
            torch.cuda.current_stream().wait_stream(side)
        values = self._parse_loss(loss)
        self._flush_writer(loss, phase)
        self._pending_choices = None
        self._close_arena()
        return values

    def _classifier_is_independent(self):
        """True when no other update of the step reads the speaker classifier C (the cyclic losses classify the converted
        and reconstructed features with it, trainer_vqvae.py:200-213 of the reference)."""
        return not self.cycle_flag

    def _classifier_stream(self, batch, phase):
        """The stream the classifier's update is enqueued on next to the rest of the step, or None (same stream, in the
        reference's order): CUDA, single process, training, C read by nobody else; config.cfg.overlap_c = 0 switches it off,
        3 keeps it in line and joins it with the speaker-adversarial net's update (update_speaker_nets)."""
        if not (phase == "train" and self.conf["use_spkr_classifier"] and not parallel.is_dist()
                and self._classifier_is_independent() and batch["in_feats"].is_cuda
                and cfg.overlap_c not in (0, 3)):
            return None
        if getattr(self, "_c_stream", None) is None:
            self._c_stream = torch.cuda.Stream(device=batch["in_feats"].device)
        return self._c_stream

    def _speaker_updates_joinable(self, batch, phase):
        """True when the speaker-adversarial net's and the classifier's updates, adjacent at the end of the step, can run
        as one set of launches (update_speaker_nets): config.cfg.overlap_c = 3, training, single process, both updates on,
        both models on FlatAdam itself (its own step()) with the same constants and no gradient clipping."""
        if not (cfg.overlap_c == 3 and phase == "train" and not parallel.is_dist() and batch["in_feats"].is_cuda
                and self.conf["use_spkradv_training"] and self.conf["use_spkr_classifier"]
                and getattr(self, "group_stack_maintenance", True)):
            return False
        from .utils import FlatAdam
        opts = [self.optimizer.get(k) for k in ("SPKRADV", "C")]
        # (the joint update stands in for both optimizers' step(): only where step IS FlatAdam's - not a subclass's, not one
        # a caller has wrapped on the instance, e.g. to look at the gradients in front of the update)
        if any(type(o) is not FlatAdam or getattr(o.step, "__func__", None) is not FlatAdam.step or o.grad_reduce_fn is not None
               for o in opts):
            return False
        if any(self.conf["optim"][k]["clip_grad_norm"] != 0 for k in ("SPKRADV", "C")):
            return False
        if any(not getattr(self.model[k], "_nets", None) for k in ("SPKRADV", "C")):
            return False
        a, b = opts
        return a.betas == b.betas and a.eps == b.eps and a.clear_grads == b.clear_grads

    def update_speaker_nets(self, batch, loss, phase="train"):
        """forward_spkradv then forward_spkrclassifier (trainer_vqvae.py:66-68 of the reference) with the two updates'
        maintenance launches shared: both forwards and cross entropies, both backward chains with their weight gradients
        and weight-norm backward left pending, then ONE launch each for the weight gradients, the weight-norm backward,
        Adam and the weight preparation of both models.  The updates read nothing of each other (SPKRADV reads G's new
        encodings, C the batch), so every value is the one the separate updates compute."""
        from ... import ops
        from .utils import flat_adam_step_many

        loss = self.forward_spkradv(batch, loss, phase=phase, step=False)
        loss = self.forward_spkrclassifier(batch, loss, phase=phase, step=False)
        names = ("C", "SPKRADV")  # (the classifier's weight-gradient workgroups, the longer ones, are dispatched first)
        models = [self.model[k] for k in names]
        for k in names:
            self.optimizer[k].zero_grad()
        for m in models:
            m.defer_wnorm = True
        try:
            for k in ("SPKRADV", "C"):
                torch.autograd.backward(loss[k], _one_like(loss[k]))
        finally:
            for m in models:
                m.defer_wnorm = False
            if any(getattr(m, "_wnorm_pending", False) for m in models):
                ops.nets_wnorm_bwd([n for m in models for n, _ in m._nets])
            for m in models:
                m._wnorm_pending = False
                m._keepalive = []
        opts = [self.optimizer[k] for k in names]
        flat_adam_step_many(opts, defer_bump=True)
        ops.nets_prepare_models([n for m in models for n, _ in m._nets],
                                [m.flat.data_ptr() + 4 * b for m in models for _, b in m._nets],
                                [m.version for m in models for _ in m._nets], [o.step_dev for o in opts])
        return loss

    def _main_update(self, batch, loss, phase):
        """The generator-side update of a step; the GAN trainers put theirs in front of it."""
        return self.forward_cycle(batch, loss, phase) if self.cycle_flag else self.forward_vqvae(batch, loss, phase)

    @torch.no_grad()
    def dev(self, batch):
        return self.train(batch, phase="dev")

    @torch.no_grad()
    def eval(self, batch):
        """Converted features for every target speaker (trainer_vqvae.py:104-119); models
        stay in training mode like the reference (quirk Q5)."""
        feats = self._feats(batch)
        out = {}
        for name in self.spkrs.keys():
            enc_h = self._get_enc_h(batch)  # the encoder always sees the SOURCE speaker's F0 (trainer_vqvae.py:107)
            dec_h, spkrvec = self._get_dec_h(batch, cv_spkr_name=name)
            out[name] = self.model["G"](feats, enc_h, dec_h, spkrvec=spkrvec)["decoded"]
        return out

    @torch.no_grad()
    def reconstruction(self, batch, tdir="reconstruction"):
        enc_h = self._get_enc_h(batch)
        dec_h, spkrvec = self._get_dec_h(batch, cv_spkr_name=None)
        return self.model["G"].forward(self._feats(batch), enc_h, dec_h, spkrvec=spkrvec)["decoded"]

    # ------------------------------------------------------------------ helpers
    def _feats(self, batch):
        return batch["raw"] if self.conf["use_raw"] else batch["in_feats"]

    def _cond(self, batch, cv=False):
        """Conditioning tensors of a batch; every sub-update of a step asks for the same ones, so they are
        built once per (batch, cv) - the batch dict is not modified during a step."""
        cache = getattr(self, "_cond_cache", None)
        if cache is None or cache[0] is not batch:
            cache = self._cond_cache = (batch, {})
        if cv not in cache[1]:
            enc_h = self._get_enc_h(batch, use_cvfeats=cv)
            dec_h, spkrvec = self._get_dec_h(batch, use_cvfeats=cv)
            cache[1][cv] = (enc_h, dec_h, spkrvec)
        return cache[1][cv]

    def _discard_grads(self, name, flag):
        m = self.model.get(name)
        if m is not None and hasattr(m, "skip_param_grads"):
            m.skip_param_grads = flag

    def _classify(self, x):
        return self.model["C"](x.transpose(1, 2)).transpose(1, 2)

    def _ce(self, logits, target):
        return self.criterion["ce"](logits.reshape(-1, logits.size(2)), target.reshape(-1))

    def _fused_ce_ok(self, model):
        """The model offers classifier + cross entropy as one op and the criterion is the stock one (ignore_index -100)."""
        ce = self.criterion["ce"]
        return hasattr(model, "forward_ce") and getattr(ce, "ignore_index", None) == -100 and \
            not cfg.separate_ce

    def _classify_ce(self, x, target):
        """_ce(_classify(x), target)"""
        C = self.model["C"]
        if self._fused_ce_ok(C):
            return self._dp_ce(C.forward_ce(x.transpose(1, 2), target), target)
        return self._ce(self._classify(x), target)

    def _dp_ce(self, value, target):
        ce = self.criterion["ce"]  # data parallel: this rank's share of the global mean (parallel._DPLoss)
        return ce.scale_ce(value, target.reshape(-1)) if hasattr(ce, "scale_ce") else value  # (the view _ce hands over)

    def _spkradv_ce(self, encoded, target, detach=False):
        """_ce(SPKRADV.forward(encoded, detach), target)"""
        S = self.model["SPKRADV"]
        if self._fused_ce_ok(S):
            return self._dp_ce(S.forward_ce(encoded, target, detach=detach), target)
        return self._ce(S.forward(encoded, detach=detach) if detach else S.forward(encoded), target)

    def step_model(self, loss, model="G"):
        m = self.model[model]
        self.optimizer[model].zero_grad()
        total = loss[model]
        # (group_stack_maintenance = False on the trainer: every stack does its own, the path a plain backward() takes)
        grouped = (getattr(self, "group_stack_maintenance", True)
                   and hasattr(m, "finish_grads"))
        if grouped:  # the model's stacks leave their weight-norm backward to ONE launch after the backward pass ...
            m.defer_wnorm = True
        # (weight-norm backward + Adam + preparation as ONE launch was built and measured in round 4: bit-identical, not
        # faster - each phase is a chain of memory round trips of its own - and removed in round 6, docs/history/round4.md)
        try:
            torch.autograd.backward(total, _one_like(total))  # (a cached 1: backward() would fill a new one every call)
        finally:
            if grouped:
                m.defer_wnorm = False
                m.finish_grads()
        if model == "G" and getattr(self, "_defer_G_tail", False) and hasattr(self.optimizer[model], "reduce_grads_start"):
            self.optimizer[model].reduce_grads_start()
            self._G_tail = lambda: self._finish_step(model, m, grouped)
            return
        if model == "C" and getattr(self, "_defer_C_tail", False) and hasattr(self.optimizer[model], "mark_reduced"):
            self._C_tail = lambda: self._finish_step(model, m, grouped)
            return
        if model == "SPKRADV" and getattr(self, "_C_tail", None) is not None and hasattr(self.optimizer[model], "mark_reduced"):
            # the speaker-adversarial net's and the classifier's gradient blocks as one exchange, then both updates
            from ... import ops
            parallel.all_reduce_many([m.grad_flat, self.model["C"].grad_flat])
            self.optimizer[model].mark_reduced()
            self.optimizer["C"].mark_reduced()
            self._finish_step(model, m, grouped)
            tail, self._C_tail = self._C_tail, None
            tail()
            return
        self._finish_step(model, m, grouped)

    def _G_step_is_last_of_main_update(self):
        """The generator's optimizer step may be moved behind the classifier's update only if nothing between them reads the
        generator's new parameters (the GAN trainers with ``train_first: G`` run the discriminator update after it)."""
        return True

    def _finish_step(self, model, m, grouped):
        clip = self.conf["optim"][model]["clip_grad_norm"]
        if clip != 0:
            # data parallel: reduce -> clip -> Adam, so that the norm is the global batch's (the reference clips the
            # gradient of its one batch, trainer_vqvae.py:203-206)
            if hasattr(self.optimizer[model], "reduce_grads"):
                self.optimizer[model].reduce_grads()
            if hasattr(m, "grad_flat"):
                flat_clip_grad_norm(m, clip)
            else:
                torch.nn.utils.clip_grad_norm_(m.parameters(), clip)
        opt = self.optimizer[model]
        if grouped and hasattr(opt, "step_dev"):
            # ... and are prepared for the new parameters in one launch as well, which also advances Adam's step count
            opt.step(defer_bump=True)
            m.prepare_nets(bump_step=opt.step_dev)
        else:
            opt.step()

    # ------------------------------------------------------------------ sub-updates
    def forward_vqvae(self, batch, loss, phase="train"):
        enc_h, dec_h, spkrvec = self._cond(batch)
        G = self.model["G"]
        # (the commitment losses come out of the quantizer op where the model offers it: one backward launch per
        # quantizer instead of two and an addition)
        kw = ({"want_commit": True, "commit_mask": batch["encoder_mask"]}
              if getattr(G, "can_commit", False) and self.conf["ema_flag"]
              and not cfg.separate_commit else {})
        outputs = G.forward(self._feats(batch), enc_h, dec_h, spkrvec=spkrvec, **kw)
        loss = self.calculate_vqvae_loss(batch, outputs, loss)
        self._discard_grads("SPKRADV", True)  # only optimizer["G"] steps here (Q7)
        if self.conf["use_spkradv_training"]:
            loss = self.calculate_spkradv_loss(batch, outputs, loss, label="org", phase=phase)
        loss.add("objective", 1.0, loss["G"])
        if phase == "train":
            self.step_model(loss, model="G")
        self._discard_grads("SPKRADV", False)
        return loss

    def forward_cycle(self, batch, loss, phase="train"):
        enc_h, dec_h, spkrvec = self._cond(batch)
        enc_h_cv, dec_h_cv, spkrvec_cv = self._cond(batch, cv=True)
        outs = self.model["G"].cycle_forward(self._feats(batch), enc_h, dec_h, enc_h_cv, dec_h_cv, spkrvec, spkrvec_cv)
        self._discard_grads("SPKRADV", True)
        self._discard_grads("C", True)
        if self.conf["use_vqvae_loss"]:
            loss = self.calculate_vqvae_loss(batch, outs[0]["org"], loss)
        loss = self.calculate_cyclevqvae_loss(batch, outs, loss)
        if self.conf["use_spkradv_training"]:
            for label in ["cv", "recon"]:
                loss = self.calculate_spkradv_loss(batch, outs[0][label], loss, label=label, phase=phase)
        loss.add("objective", 1.0, loss["G"])
        if phase == "train":
            self.step_model(loss, model="G")
        self._discard_grads("SPKRADV", False)
        self._discard_grads("C", False)
        return loss

    def forward_spkradv(self, batch, loss, phase="train", step=True):
        if not self.conf["use_spkradv_training"]:
            return loss
        enc_h, dec_h, spkrvec = self._cond(batch)
        # a full G forward whose only use is detached (EMA fires again: quirk Q4)
        grad_on = torch.is_grad_enabled()
        G = self.model["G"]
        # only the encodings are read below: the last decoder is dead code here (VQVAE2.forward; models without the
        # switch - the CPU oracle under this trainer in the tests - run the whole forward like the reference)
        kw = {"need_decoded": False} if getattr(G, "can_skip_decoder", False) else {}
        with torch.no_grad():
            outputs = G.forward(self._feats(batch), enc_h, dec_h, spkrvec=spkrvec, **kw)
        er = self.model["G"].encoder_receptive_size if self.conf["causal"] else 0
        encoded = [e[:, er:] for e in outputs["encoded_unmod"]] if er else outputs["encoded_unmod"]
        with torch.set_grad_enabled(grad_on):
            loss["SPKRADV"] = _scaled(self.conf["alpha"]["ce"], self._spkradv_ce(encoded, batch["org_h"][:, er:], detach=True))
            if phase == "train" and step:
                self.step_model(loss, model="SPKRADV")
        return loss

    def forward_spkrclassifier(self, batch, loss, phase="train", step=True):
        if not self.conf["use_spkr_classifier"]:
            return loss
        loss["C_real"] = self._classify_ce(batch["in_feats"], batch["org_h"])
        loss.add("C", self.conf["alpha"]["ce"], loss["C_real"])
        if phase == "train" and step:
            self.step_model(loss, model="C")
        return loss

    # ------------------------------------------------------------------ loss algebra
    def _commit_terms(self, outputs, emask, loss, suffix=""):
        fused = outputs.get("commit") if suffix == "" else None
        for n in range(self.conf["n_vq_stacks"]):
            enc, emb = outputs["encoded"][n], outputs["emb_idx"][n]
            if fused is not None:
                loss[f"G_commit{n}{suffix}"] = parallel.scale_masked_mean(fused[n], emask)
                continue
            loss[f"G_commit{n}{suffix}"] = self.criterion["fmse"](enc, emb.detach(), mask=emask)
            if not self.conf["ema_flag"]:
                loss[f"G_dict{n}{suffix}"] = self.criterion["fmse"](emb, enc.detach(), mask=emask)
        return loss

    def calculate_vqvae_loss(self, batch, outputs, loss):
        cs = self.conf["causal_size"]
        decoded, target, dmask = outputs["decoded"], batch["out_feats"], batch["decoder_mask"]
        fl1 = self.criterion["fl1"]
        three = fl1.recon(decoded, target, dmask, cs, self.criterion["fstft"]) if hasattr(fl1, "recon") else None
        if three is not None:  # the HIP criterion: the three terms on the decoded features as one op
            loss["G_l1"], loss["G_mse"], loss["G_stft"] = three
        else:
            loss["G_l1"] = fl1(decoded, target, mask=dmask, causal_size=cs)
            loss["G_mse"] = self.criterion["fmse"](decoded, target, mask=dmask, causal_size=cs)
            loss["G_stft"] = self.criterion["fstft"](decoded, target, causal_size=cs)
        loss = self._commit_terms(outputs, batch["encoder_mask"], loss)
        a = self.conf["alpha"]
        for k in ["l1", "mse", "stft"]:
            loss.add("G", a[k], loss[f"G_{k}"])
        for k in ["commit"] + ([] if self.conf["ema_flag"] else ["dict"]):
            for n in range(self.conf["n_vq_stacks"]):
                loss.add("G", a[k], loss[f"G_{k}{n}"])
        return loss

    def calculate_cyclevqvae_loss(self, batch, outputs, loss):
        a = self.conf["alpha"]
        cs = self.conf["causal_size"] * 2 if self.conf["causal"] else 0
        for c in range(self.conf["n_cycles"]):
            for io in ["cv", "recon"]:
                lbl = f"{c}cyc_{io}"
                o = outputs[c][io]
                if io == "cv":
                    emask = batch["encoder_mask"]
                    loss[f"C_fake_{lbl}"] = self._classify_ce(o["decoded"], batch["cv_h"])
                else:
                    emask, dmask = batch["cycle_encoder_mask"], batch["cycle_decoder_mask"]
                    tgt = batch["in_feats"]
                    fl1 = self.criterion["fl1"]
                    three = (fl1.recon(o["decoded"], tgt, dmask, cs, self.criterion["fstft"]) if hasattr(fl1, "recon")
                             else None)
                    if three is not None:
                        loss[f"G_l1_{lbl}"], loss[f"G_mse_{lbl}"], loss[f"G_stft_{lbl}"] = three
                    else:
                        loss[f"G_l1_{lbl}"] = fl1(o["decoded"], tgt, mask=dmask, causal_size=cs)
                        loss[f"G_mse_{lbl}"] = self.criterion["fmse"](o["decoded"], tgt, mask=dmask, causal_size=cs)
                        loss[f"G_stft_{lbl}"] = self.criterion["fstft"](o["decoded"], tgt, causal_size=cs)
                loss = self._commit_terms(o, emask, loss, suffix=f"_{lbl}")
        # weighting (trainer_vqvae.py:330-357)
        for c in range(self.conf["n_cycles"]):
            for io in ["cv", "recon"]:
                lbl = f"{c}cyc_{io}"
                for n in range(self.conf["n_vq_stacks"]):
                    loss.add("G", a["cycle"] * a["commit"], loss[f"G_commit{n}_{lbl}"])
                    if not self.conf["ema_flag"]:
                        loss.add("G", a["cycle"] * a["dict"], loss[f"G_dict{n}_{lbl}"])
                if io == "recon":
                    for k in ["l1", "mse", "stft"]:
                        loss.add("G", a["cycle"] * a[k], loss[f"G_{k}_{lbl}"])
                else:
                    loss.add("G", a["cycle"] * a["ce"], loss[f"C_fake_{lbl}"])
        return loss

    def calculate_spkradv_loss(self, batch, outputs, loss, label="org", phase="train"):
        er = self.model["G"].encoder_receptive_size if self.conf["causal"] else 0
        encoded = [e[:, er:] for e in outputs["encoded_unmod"]] if er else outputs["encoded_unmod"]
        loss[f"G_spkradv_{label}"] = self._spkradv_ce(encoded, batch["org_h"][:, er:])
        w = self.conf["alpha"]["ce"] * (self.conf["alpha"]["cycle"] if label == "recon" else 1)
        loss.add("G", w, loss[f"G_spkradv_{label}"])
        return loss

    def _check_cycle_start(self):
        if self.conf["use_cyclic_training"] and self.steps > self.conf["n_steps_cycle_start"]:
            self.cycle_flag = True
        if self.conf["use_cyclic_training"] and not self.conf["use_spkr_classifier"]:
            raise ValueError("use_cyclic_training requires use_spkr_classifier to be true")
