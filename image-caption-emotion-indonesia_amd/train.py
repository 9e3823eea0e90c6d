"""The training loop of the reference on the MI355X kernels.

  train_step     one iteration of the bodies of train_factual / train_emotion
                 (stylenet/train_multitask.py:373-389, 527-537; nic/train_transfer_fac.py:252-296)
  policy_step / self_critical_step / bleu_reward / DeviceBleuReward / cider_reward / DeviceCiderReward   reward-based
                 fine-tuning on sampled captions (self-critical sequence training, Rennie et al. 2017; no counterpart in the
                 reference); with a DeviceBleuReward or a DeviceCiderReward the rewards and advantages are computed on the
                 device (ops.bleu_rows, ops.cider_rows)
  train_factual  stylenet/train_multitask.py:364-408
  train_emotion  stylenet/train_multitask.py:511-557
  val_factual / val_emotion   stylenet/train_multitask.py:272-361, 411-508 (eval-mode trunk on the
                 running BN statistics, free-running decode, top-5 accuracy, BLEU-4, one beam sample)
Same order of operations: targets -> encoder -> decoder -> CrossEntropyLoss -> zero_grad ->
backward -> clip_gradient -> optimizer.step. The loss stays on the device; `.item()` is taken
once per log interval instead of every step (the reference syncs every step, :393,396).
"""
import random

import torch
import torch.nn as nn

from . import decode, ops
from .beam import Constraints, PerImage
from .metrics import CiderCorpus, corpus_bleu, corpus_cider_d, sentence_bleu, sentence_cider_d
from .utils import AverageMeter, accuracy, clip_gradient


_scale_cache = {}


def _backward(loss, loss_scale):
    """loss.backward(), or d(loss_scale * loss): the weight goes in as the incoming gradient of the
    loss kernels' backward instead of a torch multiply on the scalar."""
    if loss_scale is None:
        loss.backward()
        return
    key = (loss.device, float(loss_scale))
    g = _scale_cache.get(key)
    if g is None:
        if len(_scale_cache) > 64:
            _scale_cache.clear()
        g = torch.full((), float(loss_scale), dtype=torch.float32, device=loss.device)
        _scale_cache[key] = g
    loss.backward(g)


class CrossEntropyLoss(nn.Module):
    """nn.CrossEntropyLoss() (mean reduction) on the fused HIP softmax+NLL kernels."""

    def forward(self, outputs, targets):
        return ops.cross_entropy(outputs, targets)


def train_step(encoder, decoder, optimizer, criterion, images, captions, lengths, grad_clip,
               mode=None, zero_encoder_grad=True, teacher_forcing_ratio=0.8, tf_mask=None,
               loss_scale=None):
    """One optimisation step; returns the (device) loss tensor of this batch.

    mode=None: factual step (decoder called without `mode`, both modules zero_grad'ed).
    mode='happy'|...: emotion step; the reference leaves encoder.zero_grad() commented out
    there (train_multitask.py:534) -> pass zero_encoder_grad=False to reproduce that.
    loss_scale: data-parallel weight N_rank/N_global applied to the back-propagated loss.
    """
    targets = ops.packed_targets(captions, lengths)
    features = encoder(images)
    kw = {}
    if mode is not None:
        kw["mode"] = mode
    if tf_mask is not None:
        kw["tf_mask"] = tf_mask
    outputs = decoder(captions, lengths, features, teacher_forcing_ratio=teacher_forcing_ratio, **kw)
    loss = criterion(outputs, targets)
    decoder.zero_grad()
    if zero_encoder_grad:
        encoder.zero_grad()
    _backward(loss, loss_scale)
    clip_gradient(optimizer, grad_clip)
    optimizer.step()
    return loss.detach()


def train_step_att(encoder, decoder, optimizer, criterion, images, captions, lengths, grad_clip,
                   mode=None, zero_encoder_grad=True, teacher_forcing_ratio=0.8, tf_mask=None,
                   alpha_c=1.0, loss_scale=None):
    """One step of the attention loops (stylenet/train_multitask_att.py:398-417): inputs
    captions[:, :-1], targets captions[:, 1:], lengths-1, loss += alpha_c*((1-sum_t alpha)^2).mean().
    `lengths` are the loader's lengths (the -1 is applied here, as the reference does at :402)."""
    lengths = [l - 1 for l in lengths]
    targets = ops.packed_targets(captions[:, 1:].contiguous(), lengths)
    features = encoder(images)
    # the attention encoder has no trainable head to hang pre_head_hook on: a data-parallel
    # optimiser's overlapped update (capnet.parallel) must have landed before the decoder reads
    # the parameters
    if hasattr(optimizer, "wait_for_update"):
        optimizer.wait_for_update()
    kw = {}
    if mode is not None:
        kw["mode"] = mode
    if tf_mask is not None:
        kw["tf_mask"] = tf_mask
    outputs, alphas = decoder(captions[:, :-1].contiguous(), lengths, features,
                              teacher_forcing_ratio=teacher_forcing_ratio, **kw)
    loss = criterion(outputs, targets)
    loss = ops.attention_loss(loss, alphas, alpha_c)
    decoder.zero_grad()
    if zero_encoder_grad:
        encoder.zero_grad()
    _backward(loss, loss_scale)
    clip_gradient(optimizer, grad_clip)
    optimizer.step()
    return loss.detach()


def policy_step(decoder, optimizer, features, captions, advantages, grad_clip, mode=None, loss_scale=None):
    """One policy-gradient step on given captions: ascends sum_r advantages[r] * log p(caption r) / N, N the captions' words.
    Returns (loss, caption_logp): the (device) loss -(1/N) sum_r advantages[r] log p(caption r) and the model's
    log-probability of every caption before the update, float32 on the device in the caller's order.

    captions: a flat list of token lists [start, w_1 .. w_j] (caption r on row r of `features`) or the nested list
    sample_random returns (capnet.decode.flat_captions); advantages: one float per caption, in the same (flattened) order -- a
    list, a host tensor, or a tensor on the decoder's device, which is permuted into the batch's order there and never read
    by the host (the same float32 values, so the same loss to the last bit).
    Deterministic: every step is teacher forced, so `random` is not consumed. Order of operations: pack ->
    capnet.decode.policy_logits -> ops.policy_loss -> zero_grad -> backward -> clip_gradient -> optimizer.step.
    features: the decoder's input, not images -- no encoder parameter receives a gradient (a plain decoder does not read
    them at all; an attention decoder's trunk is frozen). mode: as train_step's; loss_scale: _backward's."""
    inputs, lengths, targets, order, feats = decode.policy_batch(decoder, features, captions)
    if torch.is_tensor(advantages) and advantages.device == inputs.device and advantages.is_cuda:
        # advantages that were formed on the device stay there: permuted into the batch's order by a gather, no host read
        if advantages.numel() != len(order):
            raise ops.CapnetError("policy_step: %d advantages for %d captions" % (advantages.numel(), len(order)))
        adv = advantages.detach().reshape(-1).to(torch.float32).index_select(
            0, torch.tensor(order, dtype=torch.int64).to(inputs.device))
    else:
        adv = [float(a) for a in (advantages.tolist() if torch.is_tensor(advantages) else advantages)]
        if len(adv) != len(order):
            raise ops.CapnetError("policy_step: %d advantages for %d captions" % (len(adv), len(order)))
        adv = torch.tensor([adv[r] for r in order], dtype=torch.float32).to(inputs.device)
    logits = decode.policy_logits(decoder, inputs, lengths, feats, mode)
    loss, logp = ops.policy_loss(logits, targets, adv, ops.batch_sizes_from_lengths(lengths))
    decoder.zero_grad()
    _backward(loss, loss_scale)
    clip_gradient(optimizer, grad_clip)
    optimizer.step()
    caption_logp = torch.empty_like(logp)
    caption_logp[torch.tensor(order, dtype=torch.int64, device=logp.device)] = logp
    return loss.detach(), caption_logp


def mean_baseline(rewards):
    """rewards [image][sample] -> baselines of the same shape: for every sample the mean reward of the image's OTHER samples
    (so an image's advantages sum to 0). Needs at least two samples per image."""
    out = []
    for row in rewards:
        if len(row) < 2:
            raise ValueError("baseline='mean' needs samples >= 2 (the mean of the other samples)")
        total = sum(row)
        out.append([(total - r) / (len(row) - 1) for r in row])
    return out


def self_critical_step(decoder, optimizer, features, reward, start_token, end_token, grad_clip, samples=5, baseline='greedy',
                       mode=None, temperature=1.0, top_k=0, top_p=1.0, seed=None, loss_scale=None, exclude=None):
    """One step of self-critical sequence training (Rennie et al., 2017): draw `samples` captions per image with
    decoder.sample_random, score them on the host with reward(image_index, tokens) -> float, subtract a baseline and take
    policy_step on the advantages.

    baseline: 'greedy' -- the reward of the image's width-1 beam caption (decoder.sample_batch(k=1)); 'mean' -- the mean
    reward of the image's other samples (samples >= 2, ValueError otherwise).
    temperature / top_k / top_p / seed are sample_random's and only shape the exploration: the gradient is always that of
    the model's own, untempered and untruncated log-probability of the drawn captions (policy_step), not of the
    distribution they were drawn from.
    exclude (a capnet.beam.Constraints without forced words; None: the step as it was) is sample_random's too and shapes the
    exploration in the same sense: no drawn caption repeats an n-gram, ends within min_words or holds a banned word, and the
    step scores none that does. The greedy baseline obeys it as well: the greedy row of the one decode on the device route,
    decoder.sample_batch(k=1, constraints=exclude) on the host route -- a width-1 beam under the same exclusions is the argmax
    over the allowed words, the same caption.
    features: as policy_step's. Returns {'loss': the device loss, 'reward_mean', 'baseline_mean', 'advantage_abs_mean':
    floats over all samples, 'zero_rows': the captions whose advantage is exactly 0 (under 'greedy': the samples that
    scored what the greedy caption did, the greedy caption itself among them)}.

    reward a DeviceBleuReward or a DeviceCiderReward: the device route. 'greedy': ONE decode,
    decoder.sample_random(greedy=True) -- the greedy caption is one more row per image of the sampled decode, not a second
    search (it is the width-1 beam's caption wherever that one reaches <end> within max_seq_length) -- and ONE reward launch
    (ops.bleu_rows or ops.cider_rows; only the first tensor reward.rows returns is used) over all n (samples + 1) rows, on
    the ids the sampler left on the device; advantage = reward[drawn] - reward[greedy row of its image], exactly 0 where the two
    float32 rewards are equal. 'mean': the same launch without the greedy row and mean_baseline's formula in fp64. The
    advantages are rounded once to float32 and policy_step takes them as a device tensor: the host reads the ids once, for
    packing, and computes no reward and no advantage. The dict's 'reward_mean', 'baseline_mean', 'advantage_abs_mean' (fp64)
    and 'zero_rows' (int64) are then 0-d device tensors -- reading one is the caller's synchronisation."""
    if baseline not in ("greedy", "mean"):
        raise ValueError("baseline %r (expected 'greedy' or 'mean')" % (baseline,))
    if baseline == "mean" and int(samples) < 2:
        raise ValueError("baseline='mean' needs samples >= 2 (the mean of the other samples)")
    kw = {} if mode is None else {"mode": mode}
    if exclude is not None and not isinstance(exclude, Constraints):     # (a PerImage too: one rule for all rows)
        raise ops.CapnetError("exclude must be a capnet.beam.Constraints, not %r" % (exclude,))
    ex, con = ({}, {}) if exclude is None else ({"exclude": exclude}, {"constraints": exclude})
    if isinstance(reward, (DeviceBleuReward, DeviceCiderReward)):
        m, greedy = int(samples), baseline == "greedy"
        drawn, ids, _ = decoder.sample_random(features, start_token, end_token, samples=m, temperature=temperature, top_k=top_k,
                                              seed=seed, top_p=top_p, device=True, greedy=greedy, **kw, **ex)
        r = reward.rows(ids, start_token, end_token, m + greedy)[0].double().view(-1, m + greedy)
        if greedy:
            drawn, base, r = [row[:m] for row in drawn], r[:, m:].expand(-1, m), r[:, :m]
        else:
            base = (r.sum(1, keepdim=True) - r) / (m - 1)
        adv = (r - base).reshape(-1)
        loss, _ = policy_step(decoder, optimizer, features, drawn, adv.to(torch.float32), grad_clip, mode=mode,
                              loss_scale=loss_scale)
        return {"loss": loss, "reward_mean": r.mean(), "baseline_mean": base.mean(), "advantage_abs_mean": adv.abs().mean(),
                "zero_rows": (adv == 0).sum()}
    drawn = decoder.sample_random(features, start_token, end_token, samples=samples, temperature=temperature, top_k=top_k,
                                  seed=seed, top_p=top_p, **kw, **ex)
    rewards = [[float(reward(i, tokens)) for tokens, _ in row] for i, row in enumerate(drawn)]
    if baseline == "mean":
        base = mean_baseline(rewards)
    else:
        greedy = decoder.sample_batch(features, start_token, end_token, k=1, **kw, **con)
        base = [[float(reward(i, [int(w) for w in g]))] * len(rewards[i]) for i, g in enumerate(greedy)]
    adv = [r - b for rr, bb in zip(rewards, base) for r, b in zip(rr, bb)]
    loss, _ = policy_step(decoder, optimizer, features, drawn, adv, grad_clip, mode=mode, loss_scale=loss_scale)
    n = float(len(adv))
    return {"loss": loss,
            "reward_mean": sum(r for rr in rewards for r in rr) / n,
            "baseline_mean": sum(b for bb in base for b in bb) / n,
            "advantage_abs_mean": sum(abs(a) for a in adv) / n,
            "zero_rows": sum(1 for a in adv if a == 0.0)}


def bleu_reward(references, weights=(0.25, 0.25, 0.25, 0.25)):
    """A ready-made `reward` for self_critical_step: reward(i, tokens) = corpus_bleu of the one sentence `tokens` against
    references[i], the list of reference token lists of image i. Tokens are taken as evaluate() takes them: as they are,
    <start> / <end> included on both sides."""
    def reward(i, tokens):
        return corpus_bleu([references[i]], [[int(w) for w in tokens]], weights=weights)
    return reward


def pack_references(references, who="pack_references"):
    """references [image][reference][word] -> (refs int32 [n, R, Lr] zero padded, ref_len int32 [n, R]) on the host: R
    the most references of an image, Lr the longest reference; an image with fewer references, or an empty one among
    them, has slots of length 0, which the kernels skip. The one packing of DeviceBleuReward and DeviceCiderReward; `who`
    names the caller in the ValueErrors."""
    if not len(references):
        raise ValueError("%s: no images" % who)
    R = max(len(refs) for refs in references)
    Lr = max([len(r) for refs in references for r in refs] + [0])
    if any(not any(len(r) for r in refs) for refs in references):
        raise ValueError("%s: every image needs at least one non-empty reference" % who)
    if R > ops.BLEU_MAX_REFS or R * Lr > ops.BLEU_MAX_REF_WORDS:
        raise ValueError("%s: %d references of up to %d words (at most %d references, %d padded words per "
                         "image)" % (who, R, Lr, ops.BLEU_MAX_REFS, ops.BLEU_MAX_REF_WORDS))
    refs = torch.zeros((len(references), R, Lr), dtype=torch.int32)
    ref_len = torch.zeros((len(references), R), dtype=torch.int32)
    for i, rr in enumerate(references):
        for j, r in enumerate(rr):
            if len(r):
                refs[i, j, :len(r)] = torch.tensor(r, dtype=torch.int32)
                ref_len[i, j] = len(r)
    return refs, ref_len


class DeviceBleuReward(object):
    """bleu_reward whose arithmetic can stay on the device: sentence BLEU (capnet.metrics.sentence_bleu; smooth=1: add-one
    on n >= 2, so a caption without a matching 4-gram still scores) against references[i], the reference token lists of
    image i, taken as they are. The references are packed once (pack) and uploaded once per device; rows() scores every
    row of a sampled decode there (ops.bleu_rows). Called as reward(i, tokens) it is a host reward like bleu_reward's, so
    it serves wherever one does. self_critical_step takes the device route for it (see there).
    Every image needs at least one non-empty reference; at most ops.BLEU_MAX_REFS references per image and
    ops.BLEU_MAX_REF_WORDS words in an image's padded block (references x the longest reference): ValueError beyond."""

    def __init__(self, references, weights=(0.25, 0.25, 0.25, 0.25), smooth=0, device=None):
        if len(weights) != 4:
            raise ValueError("DeviceBleuReward: four weights (BLEU-1 .. BLEU-4), not %d" % len(weights))
        if smooth not in (0, 1):
            raise ValueError("smooth %r (0: none, 1: add one for n >= 2)" % (smooth,))
        self.references = [[[int(w) for w in r] for r in refs] for refs in references]
        self.weights, self.smooth = tuple(float(w) for w in weights), int(smooth)
        self.refs, self.ref_len = self.pack(self.references)
        self._on = {}
        if device is not None:
            self.on(device)

    @staticmethod
    def pack(references):
        """pack_references(references): (refs int32 [n, R, Lr] zero padded, ref_len int32 [n, R]) on the host."""
        return pack_references(references, "DeviceBleuReward")

    def on(self, device):
        """(refs, ref_len) on `device`, uploaded at the first call for it."""
        device = torch.device(device)
        if device not in self._on:
            self._on[device] = (self.refs.to(device), self.ref_len.to(device))
        return self._on[device]

    def __call__(self, i, tokens):
        return sentence_bleu(self.references[i], [int(w) for w in tokens], self.weights, self.smooth)

    def rows(self, ids, start_token, end_token, per_image):
        """(reward float32 [rows], stats int32 [rows, 10]) on the device for the ids [images x per_image, steps] of a
        sampled decode of all the images, in order (ops.bleu_rows)."""
        if ids.shape[0] != len(self.references) * int(per_image):
            raise ops.CapnetError("DeviceBleuReward: %d rows for %d images x %d" % (ids.shape[0], len(self.references), per_image))
        refs, ref_len = self.on(ids.device)
        return ops.bleu_rows(ids, start_token, end_token, per_image, refs, ref_len, self.weights, self.smooth)


def cider_reward(references, corpus=None, sigma=6.0):
    """bleu_reward's counterpart for CIDEr-D: reward(i, tokens) = capnet.metrics.sentence_cider_d of `tokens` against
    references[i], in [0, 10]. corpus: the capnet.metrics.CiderCorpus whose document frequencies weigh the n-grams (normally
    the training set's); None: one built from `references`. Tokens are taken as they are."""
    corpus = CiderCorpus(references) if corpus is None else corpus

    def reward(i, tokens):
        return sentence_cider_d(corpus, references[i], [int(w) for w in tokens], sigma)
    return reward


class DeviceCiderReward(object):
    """cider_reward whose arithmetic can stay on the device, with DeviceBleuReward's interface: CIDEr-D
    (capnet.metrics.sentence_cider_d, in [0, 10]) against references[i], the reference token lists of image i of the batch,
    taken as they are. corpus: a capnet.metrics.CiderCorpus, normally built once from the whole training set and shared by
    the reward objects of every batch (its tables are uploaded once per device); None: one built from `references`. The
    references are packed once (pack_references), and the norm of every reference's tf-idf vector is computed here, on the
    host, once (ref_norm float64 [images, R, 4]); rows() scores every row of a sampled decode on the device
    (ops.cider_rows). Called as reward(i, tokens) it is a host reward. self_critical_step takes the device route for it.
    The limits on the references are DeviceBleuReward's: ValueError beyond."""

    def __init__(self, references, corpus=None, sigma=6.0, device=None):
        if not float(sigma) > 0.0:
            raise ValueError("sigma %r (must be positive)" % (sigma,))
        self.references = [[[int(w) for w in r] for r in refs] for refs in references]
        self.refs, self.ref_len = self.pack(self.references)
        self.corpus = CiderCorpus(self.references) if corpus is None else corpus
        self.sigma = float(sigma)
        self.ref_norm = torch.zeros(tuple(self.ref_len.shape) + (4,), dtype=torch.float64)
        for i, rr in enumerate(self.references):
            for j, r in enumerate(rr):
                if len(r):
                    self.ref_norm[i, j] = torch.tensor(self.corpus.vectors(r)[1], dtype=torch.float64)
        self._on = {}
        if device is not None:
            self.on(device)

    @staticmethod
    def pack(references):
        """pack_references(references): (refs int32 [n, R, Lr] zero padded, ref_len int32 [n, R]) on the host."""
        return pack_references(references, "DeviceCiderReward")

    def on(self, device):
        """(refs, ref_len, ref_norm, the corpus' tables) on `device`, uploaded at the first call for it."""
        device = torch.device(device)
        if device not in self._on:
            self._on[device] = (self.refs.to(device), self.ref_len.to(device), self.ref_norm.to(device), self.corpus.on(device))
        return self._on[device]

    def __call__(self, i, tokens):
        return sentence_cider_d(self.corpus, self.references[i], [int(w) for w in tokens], self.sigma)

    def rows(self, ids, start_token, end_token, per_image):
        """(reward float32 [rows], parts float64 [rows, 4], stats int32 [rows, 9]) on the device for the ids
        [images x per_image, steps] of a sampled decode of all the images, in order (ops.cider_rows)."""
        if ids.shape[0] != len(self.references) * int(per_image):
            raise ops.CapnetError("DeviceCiderReward: %d rows for %d images x %d" % (ids.shape[0], len(self.references), per_image))
        refs, ref_len, ref_norm, tables = self.on(ids.device)
        return ops.cider_rows(ids, start_token, end_token, per_image, refs, ref_len, ref_norm, tables, self.corpus.log_n,
                              self.sigma)


class TrunkPipeline(object):
    """Software pipeline over training steps: the frozen trunks of the next `depth` batches run on
    their own streams while head + decoder + loss + backward + clamp + Adam of the current batch
    run on a side stream.

    The ResNet-152 trunk runs under no_grad and none of its inputs depend on the parameter update
    (stylenet/model.py:23-25; train_multitask.py:163-167 only optimises the head and the decoder),
    so this reorders nothing that is ordered in the reference: every step sees exactly the
    parameters and random draws of the sequential loop and produces the same numbers; the BatchNorm
    running statistics of the trunk are updated once per pass, in pass order (the passes defer the
    update and an event chain orders it, capnet_trunk_update_running). What it changes:
      * the decoder's many small, latency-bound launches share the chip with the convolutions of
        the following batches instead of leaving it idle;
      * `depth` (default 3) trunk passes are in flight: while one sits in a launch-bound bubble
        (bn_finalize, tail fix-ups: tiny kernels between the convolutions) the convolutions of
        another one run (tools/probes/trunk_overlap_probe.py: 17.0 -> 15.2-16.0 ms per pass with two;
        measured step time 18.9 / 16.1 / 15.7 / 16.8 ms at depth 1 / 2 / 3 / 4).

        pipe = TrunkPipeline(encoder, decoder, optimizer, criterion, grad_clip)
        for k in range(pipe.depth): pipe.prefetch(images_k)      # up to `depth` batches ahead
        for i in range(n):
            loss = pipe.step(captions_i, lengths_i, next_images=images_{i+depth} or None)
        pipe.finish()            # before reading a loss or the parameters on the caller's stream
    """

    def __init__(self, encoder, decoder, optimizer, criterion, grad_clip, attention=False,
                 alpha_c=1.0, depth=3, shared_chip_tuning=True, graph_trunk=False):
        self.encoder, self.decoder, self.optimizer = encoder, decoder, optimizer
        self.criterion, self.grad_clip = criterion, grad_clip
        self.attention, self.alpha_c = attention, alpha_c
        self.depth = max(1, int(depth))
        # shared_chip_tuning: with several passes in flight the trunk drops the K-sliced tail
        # balancing and prefers the 128x64 conv tile on the large layers (csrc/trunk.cpp; +4 %
        # images/s). Both only change the ORDER of fp32 additions (BatchNorm partial sums, K slices),
        # so results differ from the sequential loop at rounding level; False keeps the sequential
        # schedule's kernels and reproduces its numbers exactly.
        self.balance_tails = not (shared_chip_tuning and self.depth >= 2)
        # graph_trunk: replay each trunk pass (~330 launches, fixed arguments) from a hipGraph
        # captured per slot. It removes ~3.5 ms of launch calls per pass from the host, but the step
        # is bound by the GPU (the host runs ahead until the queues are full), so it measured no
        # gain on one GPU: 4370 vs 4355 images/s; off by default.
        self.graph_trunk = bool(graph_trunk)
        # The trainable half gets the HIGH-priority stream: its launches are small (a few
        # workgroups, microseconds) and form a long dependent chain, so they must be dispatched as
        # soon as they are ready; a convolution of the trunk has thousands of workgroups queued and
        # loses nothing by yielding a few slots.
        self.side = torch.cuda.Stream(priority=-1)
        self.trunk_streams = [torch.cuda.Stream() for _ in range(self.depth)]
        self._queue = []          # prefetched batches, oldest first: (features, ready event)
        self._issued = 0
        self._stats_done = None   # event after the previous pass's running-statistics update

    def prefetch(self, images):
        """Enqueue the trunk of `images` (ordered after the caller's current stream)."""
        if len(self._queue) >= self.depth:
            raise RuntimeError("TrunkPipeline: %d batches already in flight" % len(self._queue))
        slot = self._issued % self.depth
        self._issued += 1
        stream = self.trunk_streams[slot]
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            if self.attention:
                feats, apply_stats = self.encoder(images, slot=slot, defer_stats=True,
                                                  balance_tails=self.balance_tails, graph=self.graph_trunk)
            else:
                feats, apply_stats = self.encoder.trunk_features(images, slot=slot, defer_stats=True,
                                                                 balance_tails=self.balance_tails, graph=self.graph_trunk)
            ready = torch.cuda.Event()
            ready.record()
            if apply_stats is not None:
                # running statistics: after the previous pass's update, whatever stream it ran on
                if self._stats_done is not None:
                    stream.wait_event(self._stats_done)
                apply_stats()
                self._stats_done = torch.cuda.Event()
                self._stats_done.record()
        images.record_stream(stream)
        feats.record_stream(self.side)
        self._queue.append((feats, ready))

    def step(self, captions, lengths, next_images=None, mode=None, tf_mask=None, loss_scale=None,
             teacher_forcing_ratio=0.8, zero_encoder_grad=True):
        if not self._queue:
            raise RuntimeError("TrunkPipeline.step() without a prefetched batch")
        feats, ready = self._queue.pop(0)
        if next_images is not None:
            self.prefetch(next_images)      # queued before the decoder work of this batch
        enc, dec = self.encoder, self.decoder
        kw = {}
        if mode is not None:
            kw["mode"] = mode
        if tf_mask is not None:
            kw["tf_mask"] = tf_mask
        # `captions` was produced on the caller's stream (an H2D copy in the loops): order the side
        # stream after it, and keep its memory from being handed out again while the side stream
        # (up to `depth` steps behind the host) still reads it
        self.side.wait_stream(torch.cuda.current_stream())
        captions.record_stream(self.side)
        with torch.cuda.stream(self.side):
            self.side.wait_event(ready)
            if self.attention:
                if hasattr(self.optimizer, "wait_for_update"):
                    self.optimizer.wait_for_update()
                lens = [l - 1 for l in lengths]
                targets = ops.packed_targets(captions[:, 1:].contiguous(), lens)
                outputs, alphas = dec(captions[:, :-1].contiguous(), lens, feats,
                                      teacher_forcing_ratio=teacher_forcing_ratio, **kw)
                loss = self.criterion(outputs, targets)
                loss = ops.attention_loss(loss, alphas, self.alpha_c)
            else:
                targets = ops.packed_targets(captions, lengths)
                if enc.pre_head_hook is not None:
                    enc.pre_head_hook()
                features = enc.bn(enc.linear(feats))
                outputs = dec(captions, lengths, features,
                              teacher_forcing_ratio=teacher_forcing_ratio, **kw)
                loss = self.criterion(outputs, targets)
            dec.zero_grad()
            if zero_encoder_grad:
                enc.zero_grad()
            _backward(loss, loss_scale)
            clip_gradient(self.optimizer, self.grad_clip)
            self.optimizer.step()
            loss = loss.detach()
        return loss

    def in_flight(self):
        return len(self._queue)

    def finish(self):
        """Make the caller's stream wait for everything queued by the pipeline."""
        cur = torch.cuda.current_stream()
        cur.wait_stream(self.side)
        for s in self.trunk_streams:
            cur.wait_stream(s)


def _drain(pending, meter):
    for loss, n in pending:
        meter.update(loss.item(), n)
    del pending[:]


def _pipelined_loop(pipe, loader, device, step_kwargs):
    """Yields (i, loss, lengths): keeps `pipe.depth` batches prefetched ahead of the step.
    step_kwargs: dict, or callable(step index) -> dict (e.g. an explicit tf_mask per step)."""
    it = iter(loader)
    meta = []

    def feed():
        try:
            images, captions, lengths, _ = next(it)
        except StopIteration:
            return False
        captions = captions.to(device, non_blocking=True)      # before prefetch's wait_stream
        pipe.prefetch(images.to(device, non_blocking=True))
        meta.append((captions, lengths))
        return True

    for _ in range(pipe.depth):
        if not feed():
            break
    i = 0
    while meta:
        captions, lengths = meta.pop(0)
        loss = pipe.step(captions, lengths, **(step_kwargs(i) if callable(step_kwargs) else step_kwargs))
        feed()
        yield i, loss, lengths
        i += 1


def train_factual(encoder, decoder, optimizer, criterion, data_loader, log_step, grad_clip,
                  device=None, pipeline=True):
    """stylenet/train_multitask.py:364-408. pipeline=True overlaps each batch's trainable half with
    the trunks of the following batches (TrunkPipeline); the numbers are those of the sequential
    loop."""
    decoder.train()
    encoder.train()
    losses = AverageMeter()
    pending = []
    device = device or next(decoder.parameters()).device
    if pipeline:
        pipe = TrunkPipeline(encoder, decoder, optimizer, criterion, grad_clip)
        steps = _pipelined_loop(pipe, data_loader, device, {})
    else:
        pipe = None
        steps = ((i, train_step(encoder, decoder, optimizer, criterion,
                                images.to(device, non_blocking=True),
                                captions.to(device, non_blocking=True), lengths, grad_clip), lengths)
                 for i, (images, captions, lengths, _) in enumerate(data_loader))
    for i, loss, lengths in steps:
        pending.append((loss, sum(lengths)))
        if i % log_step == 0:
            if pipe is not None:
                pipe.finish()
            _drain(pending, losses)
            ops.check_device_errors(recover_lstm_timeout=True)
            print("""Step [{}/{}], [FAC], Loss: {:.4f}""".format(i, len(data_loader), losses.val))
    if pipe is not None:
        pipe.finish()
    _drain(pending, losses)
    ops.check_device_errors(recover_lstm_timeout=True)
    return losses.avg


def train_emotion(encoder, decoder, optimizer, criterion, data_loaders, tags, log_step,
                  grad_clip, device=None, pipeline=True):
    """stylenet/train_multitask.py:511-557 (emotion order drawn with random.sample, as there)."""
    decoder.train()
    encoder.train()
    losses = [AverageMeter() for _ in range(len(tags))]
    device = device or next(decoder.parameters()).device
    pipe = TrunkPipeline(encoder, decoder, optimizer, criterion, grad_clip) if pipeline else None
    for j in random.sample([i for i in range(len(tags))], len(tags)):
        pending = []
        if pipe is not None:
            steps = _pipelined_loop(pipe, data_loaders[j], device,
                                    {"mode": tags[j], "zero_encoder_grad": False})
        else:
            steps = ((i, train_step(encoder, decoder, optimizer, criterion,
                                    images.to(device, non_blocking=True),
                                    captions.to(device, non_blocking=True), lengths, grad_clip,
                                    mode=tags[j], zero_encoder_grad=False), lengths)
                     for i, (images, captions, lengths, _) in enumerate(data_loaders[j]))
        for i, loss, lengths in steps:
            pending.append((loss, sum(lengths)))
            if i % log_step == 0:
                if pipe is not None:
                    pipe.finish()
                _drain(pending, losses[j])
                ops.check_device_errors(recover_lstm_timeout=True)
                print("""Step [{}/{}], [{}], Loss: {:.4f}""".format(
                    i, len(data_loaders[j]), tags[j][:3].upper(), losses[j].val))
        if pipe is not None:
            pipe.finish()
        _drain(pending, losses[j])
    ops.check_device_errors(recover_lstm_timeout=True)
    return [l.avg for l in losses]


def _unpack_predictions(outputs, batch_sizes, lengths):
    """Per-sample argmax word ids from packed logits: the `pad_packed_sequence` + `torch.max(s, 1)`
    + `[:l]` of stylenet/train_multitask.py:311-329 (one argmax kernel over all N rows, then host
    index arithmetic)."""
    pred = ops.argmax_rows(outputs).tolist()
    off = [0]
    for b in batch_sizes:
        off.append(off[-1] + b)
    out = []
    for i, l in enumerate(lengths):
        out.append([pred[off[t] + i] for t in range(l)])
    return out


def _validate(encoder, decoder, vocab, criterion, data_loader, mode, device):
    decoder.eval()
    encoder.eval()
    import time
    from .utils import AverageMeter as _AM
    batch_time, losses, top5accs = _AM(), _AM(), _AM()
    t0 = time.time()
    references, hypotheses = [], []
    device = device or next(decoder.parameters()).device
    start, end = vocab.word2idx['<start>'], vocab.word2idx['<end>']
    features = None
    kw = {} if mode is None else {"mode": mode}
    for i, (images, captions, lengths, all_captions) in enumerate(data_loader):
        images = images.to(device)
        captions = captions.to(device)
        targets = ops.packed_targets(captions, lengths)
        with torch.no_grad():
            features = encoder(images)
            outputs = decoder(captions, lengths, features, teacher_forcing_ratio=0, **kw)
            loss = criterion(outputs, targets)
        losses.update(loss.item(), sum(lengths))
        top5accs.update(accuracy(outputs, targets, 5), sum(lengths))
        batch_time.update(time.time() - t0)
        for caps in all_captions:
            caps = [[int(w) for w in (c.tolist() if hasattr(c, "tolist") else c)] for c in caps]
            references.append([[w for w in c if w != start and w != end] for c in caps])
        for pred in _unpack_predictions(outputs, ops.batch_sizes_from_lengths(lengths), lengths):
            hypotheses.append([w for w in pred if w != start and w != end])
        assert len(references) == len(hypotheses)
    ops.check_device_errors()
    bleu4 = corpus_bleu(references, hypotheses)
    feature = features[0].unsqueeze(0)
    sampled_ids = decoder.sample(feature, start_token=start, end_token=end, **kw)[0].tolist()
    sampled_caption = []
    for word_id in sampled_ids:
        word = vocab.idx2word[word_id]
        sampled_caption.append(word)
        if word == '<end>':
            break
    print(sampled_caption)
    return batch_time.val, top5accs.avg, losses.avg, bleu4


def val_factual(encoder, decoder, vocab, criterion, data_loader, device=None):
    """stylenet/train_multitask.py:272-361. Returns (batch_time, top-5 accuracy %, loss, BLEU-4)."""
    from .nic_model import DecoderRNN
    return _validate(encoder, decoder, vocab, criterion, data_loader,
                     None if isinstance(decoder, DecoderRNN) else "factual", device)


def val_emotion(encoder, decoder, vocab, criterion, data_loaders, tags, device=None):
    """stylenet/train_multitask.py:411-508: one validation pass per emotion loader, decoded in that
    emotion's mode. Returns (batch_time, [top5 per tag], [loss per tag], [bleu4 per tag])."""
    res = [_validate(encoder, decoder, vocab, criterion, data_loaders[j], tags[j], device)
           for j in range(len(tags))]
    return (res[-1][0] if res else 0.0, [r[1] for r in res], [r[2] for r in res],
            [r[3] for r in res])


def evaluate(encoder, decoder, vocab, data_loader, mode='factual', k=5, device=None, verbose=False, on_device=False,
             one_call=False, cider=False, constraints=None, diversity=None):
    """The test-set evaluator, stylenet/evaluator.py:55-120: encoder + decoder in eval mode, every test image decoded by
    beam search, corpus BLEU-1..4 with the reference's four weight tuples (references and hypotheses as the reference
    builds them: the captions' and the sampled ids as they are, <start> / <end> included). The reference calls
    decoder.sample() per image; here a loader batch is decoded at once (decoder.sample_batch: B x k rows per step) --
    the same sequences (tests/test_sample_gpu.py). on_device / one_call: passed on to the decoder (capnet.decode.beam_decode).
    constraints: a capnet.beam.Constraints, passed on likewise (None: the calls as they were); or a capnet.beam.PerImage over
    the whole loader in image order, every batch decoded under its slice -- CapnetError where the loader holds more images than
    it has entries (at that batch) or fewer (at the end).
    diversity: a capnet.beam.Diversity, passed on likewise; the metrics are taken on the winner over all groups.
    Returns (bleu_1, bleu_2, bleu_3, bleu_4); with cider=True a fifth entry, the mean CIDEr-D of the decoded captions
    (capnet.metrics.corpus_cider_d, the corpus being the loader's own references, as the COCO scorer takes a test split)."""
    decoder.eval()
    encoder.eval()
    device = device or next(decoder.parameters()).device
    start, end = vocab.word2idx['<start>'], vocab.word2idx['<end>']
    kw = {} if mode is None else {"mode": mode}
    if on_device:
        kw["on_device"] = True
    if one_call:
        kw["one_call"] = True
    per_image = constraints if isinstance(constraints, PerImage) else None
    if constraints is not None and per_image is None:
        kw["constraints"] = constraints
    if diversity is not None:
        kw["diversity"] = diversity
    references, hypotheses = [], []
    for images, captions, lengths, all_captions in data_loader:
        with torch.no_grad():
            features = encoder(images.to(device))
        if per_image is not None:       # this batch's entries, in image order
            i0, i1 = len(hypotheses), len(hypotheses) + features.size(0)
            if i1 > len(per_image):
                raise ops.CapnetError("evaluate: a PerImage of %d entries, and the loader is at image %d" % (len(per_image), i1))
            kw["constraints"] = per_image[i0:i1]
        if per_image is not None and not hasattr(decoder, "sample_batch"):
            seqs = [decoder.sample(features[i:i + 1], start_token=start, end_token=end, k=k,
                                   **dict(kw, constraints=per_image[i0 + i]))[0].tolist() for i in range(features.size(0))]
        elif hasattr(decoder, "sample_batch"):
            seqs = decoder.sample_batch(features, start_token=start, end_token=end, k=k, **kw)
        else:       # (a decoder without one: image by image, as the reference does)
            seqs = [decoder.sample(features[i:i + 1], start_token=start, end_token=end, k=k, **kw)[0].tolist()
                    for i in range(features.size(0))]
        for sampled_ids, caps in zip(seqs, all_captions):
            caps = [[int(w) for w in (c.tolist() if hasattr(c, "tolist") else c)] for c in caps]
            references.append(caps)
            hypotheses.append([int(w) for w in sampled_ids])
            if verbose:
                for name, ids in (("ref", caps[0]), ("pred", sampled_ids)):
                    words = []
                    for word_id in ids:
                        words.append(vocab.idx2word[word_id])
                        if words[-1] == '<end>':
                            break
                    print(name, ' '.join(words))
    assert len(references) == len(hypotheses)
    if per_image is not None and len(per_image) != len(hypotheses):
        raise ops.CapnetError("evaluate: a PerImage of %d entries for a loader of %d images" % (len(per_image), len(hypotheses)))
    ops.check_device_errors()
    out = _scores(references, hypotheses, cider)
    if verbose:
        for i, b in enumerate(out[:4]):
            print('BLEU-%d' % (i + 1), b)
        if cider:
            print('CIDEr-D', out[4])
    return out


def _scores(references, hypotheses, cider=False):
    """evaluate's tuple: corpus BLEU-1..4 with the reference's four weight tuples, and with `cider` the corpus_cider_d mean."""
    out = tuple(corpus_bleu(references, hypotheses, weights=w)
                for w in ((1, 0, 0, 0), (0.5, 0.5, 0, 0), (0.33, 0.33, 0.33, 0), (0.25, 0.25, 0.25, 0.25)))
    return out + (corpus_cider_d(references, hypotheses)[0],) if cider else out


MODES = ("factual", "happy", "sad", "angry")


def evaluate_styles(encoder, decoder, vocab, data_loader, modes=MODES, k=5, device=None):
    """evaluate() in every style of `modes` on ONE pass over the loader -> {mode: (bleu_1, bleu_2, bleu_3, bleu_4)}, each
    tuple equal to evaluate(..., mode=mode, one_call=True). Per loader batch the encoder runs once (evaluate per mode runs
    it len(modes) times on the same images) and the decoder makes one sample_styles call. An image's references
    (the loader's all_captions entry) are a list of captions, shared by every mode, or a dict mode -> list."""
    decoder.eval()
    encoder.eval()
    device = device or next(decoder.parameters()).device
    start, end = vocab.word2idx['<start>'], vocab.word2idx['<end>']
    modes = tuple(modes)
    references, hypotheses = {m: [] for m in modes}, {m: [] for m in modes}
    for images, captions, lengths, all_captions in data_loader:
        with torch.no_grad():
            features = encoder(images.to(device))
        styled = decoder.sample_styles(features, start_token=start, end_token=end, k=k, modes=modes)
        for m in modes:
            for sampled_ids, caps in zip(styled[m], all_captions):
                caps = caps[m] if isinstance(caps, dict) else caps
                references[m].append([[int(w) for w in (c.tolist() if hasattr(c, "tolist") else c)] for c in caps])
                hypotheses[m].append([int(w) for w in sampled_ids])
    ops.check_device_errors()
    return {m: _scores(references[m], hypotheses[m]) for m in modes}
