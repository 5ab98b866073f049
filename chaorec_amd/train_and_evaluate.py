"""Train / evaluate loop for the hot-path models (reference train_and_evaluate.py:25-48, :516-520, :523-686).

Kept: the generic (users, pos, neg) branch, the MMGCN (user_tensor, item_tensor) branch, FREEDOM's
pre_epoch_processing hook, per-epoch gene_ranklist + val/test metrics at K in topk, early stopping on test
Recall@max(topk) with patience 20, the same log lines.  Changed: the per-batch `loss.item()` host sync
(reference :48) becomes one device-side accumulation and a single .item() per epoch.
What a model's name decides here is read from its row of registry.MODELS; the loops of their own are in epochs.py."""
import logging
import os

import torch

from . import epochs as _epochs          # (train_and_evaluate() has a parameter named epochs)
from .registry import spec_of
from .utils import EarlyStopping, EvalLists, gene_metrics, gene_metrics_device


def train(model, train_loader, optimizer, model_name="LightGCN", graphed=None):
    """One epoch.  `graphed` (optim.GraphedTrainStep) replays the captured step for full-size batches."""
    model.train()
    spec = spec_of(model_name)
    if spec.epoch is not None:
        return spec.epoch(model, train_loader, optimizer)
    if graphed is not None and getattr(graphed, "draws_in_launch", False):
        return _epochs._train_epoch_in_launch(model, train_loader, optimizer, graphed)
    sum_loss = None
    build_item_graph = True
    for batch in train_loader:
        if graphed is not None:
            d = graphed(*batch)
        else:
            optimizer.zero_grad()
            if spec.before_step is not None:
                spec.before_step(model)      # (NCL, VGCL: clustering before EVERY batch)
            if spec.build_first:
                loss = model.loss(*batch, build_item_graph=build_item_graph)
                build_item_graph = False
            else:
                loss = model.loss(*batch)
            loss.backward()
            optimizer.step()
            d = loss.detach()
        sum_loss = d.clone() if sum_loss is None else sum_loss.add_(d)
    return float(sum_loss.item()) if sum_loss is not None else 0.0


def evaluate(model, data, ranklist, topk):
    """train_and_evaluate.py:655-659.  `data` may be an EvalLists and `ranklist` a device tensor: the metrics are then
    computed in HBM (chaorec_rank_metrics_f64), otherwise by the host restatement."""
    model.eval()
    with torch.no_grad():
        if isinstance(data, EvalLists):
            return gene_metrics_device(data, ranklist, topk)
        return gene_metrics(data, ranklist, topk)


MAX_TOPK = 1024          # ops_wide.WIDE_K: the widest rank list the selection and the metric kernels take
DEFAULT_COLUMNS = 50     # gene_ranklist()'s default width (Model/LightGCN.py:137)


def _rank_list(model, kmax, on_device):
    """The evaluation's rank list, wide enough for the largest cut-off: the model's default 50 columns, or kmax of them."""
    if kmax <= DEFAULT_COLUMNS:
        return model.gene_ranklist(to_cpu=False) if on_device else model.gene_ranklist()
    return model.gene_ranklist(topk=kmax, to_cpu=False) if on_device else model.gene_ranklist(topk=kmax)


def _log_metrics(title, metrics):
    logging.info(title)
    for k, m in metrics.items():
        logging.info(f"{k}: {' | '.join(f'{name}: {value:.5f}' for name, value in m.items())}")


def _capture_step(model, train_loader, optimizer, model_name):
    """The launch-bound inner loop (train_and_evaluate.py:43-48) as one hipGraph replay per batch: possible when the
    batches already live in HBM with a fixed shape, the optimizer's step counter is on the device and the graph
    graph arrays keep their addresses between epochs (FREEDOM re-prunes its adjacency every epoch IN PLACE, so its
    step is captured once, after the first pre_epoch_processing())."""
    from .dataload import DeviceBatchSampler
    from .optim import FusedAdam, GraphedTrainStep
    if not isinstance(train_loader, DeviceBatchSampler) or not isinstance(optimizer, FusedAdam):
        return None
    spec = spec_of(model_name)
    if not spec.capture and model_name not in os.environ.get("CHAOREC_TRY_CAPTURE", "").split(","):
        return None
    if spec.pre_epoch and not getattr(model, "prunes_in_place", False):
        return None          # a graph that is re-allocated every epoch cannot sit behind captured addresses
    if len(train_loader) < 2:
        return None
    if hasattr(model, "loss_drawn") and spec.batch != "pairs" and not spec.pre_epoch:
        # the batch is drawn by the fused BPR forward itself: a replay takes no inputs at all.  The capture's warm-up
        # steps draw full batches from the epoch permutation: the edge list must hold them (the kernel clamps a read
        # past the end, but those would not be the sampler's batches), and the loader's counters / generator are put
        # back afterwards so that a captured run draws exactly what an eager one draws.
        E, B = train_loader.edges.shape[0], train_loader.batch_size
        if E < 4 * B:
            return None
        gen_state = train_loader.gen.get_state()
        train_loader.begin_epoch()
        saved = [t.clone() for t in (train_loader.step_dev, train_loader.perm_pos, train_loader.perm)]
        from .Model import LightGCN
        if type(model) is LightGCN and model.n_layers >= 1 and len(optimizer.param_groups) == 1:
            from .optim import FusedLightGCNStep
            acc = torch.zeros(1, dtype=torch.float32, device=train_loader.edges.device)
            # steps per replay: a divisor of the steps that run as whole replays.  With the light forward (by size: large
            # graphs) FusedLightGCNStep.run(E // B, full_last=True) runs E // B - 1 light steps and one full step, so the
            # divisor is taken of E // B - 1 (a divisor of E // B left k - 1 steps per epoch to single replays)
            light = FusedLightGCNStep.frontier_modes(model.num_user + model.num_item, model.n_layers,
                                                     model.user_embedding.weight.shape[1])[2]
            n_rep = E // B - 1 if (light and E % B == 0) else E // B
            k = next((c for c in (11, 10, 8, 7, 5, 4, 3, 2) if n_rep % c == 0), 1)
            g = FusedLightGCNStep(model, optimizer, batch_size=B, edges=train_loader.edges, seed=train_loader.seed,
                                  step_dev=train_loader.step_dev, perm=train_loader.perm, perm_pos=train_loader.perm_pos,
                                  loss_accum=acc, steps_per_replay=k)
            g.fused = True
        else:
            g = GraphedTrainStep(model, optimizer, batch_fn=lambda: (), loss_fn=train_loader.drawn_loss_fn(model))
        with torch.no_grad():
            for dst, src in zip((train_loader.step_dev, train_loader.perm_pos, train_loader.perm), saved):
                dst.copy_(src)
        train_loader.gen.set_state(gen_state)
        g.draws_in_launch = True
        return g
    example = next(iter(train_loader))
    return GraphedTrainStep(model, optimizer, example_batch=example)


def train_and_evaluate(model, train_loader, val_data, test_data, optimizer, epochs, model_name="LightGCN",
                       topk=(5, 10, 20), patience=20, graph=True, history=None):
    """history (optional list): receives one dict per epoch -- epoch, loss (the summed batch losses, what the reference
    logs as "Epoch n, Loss"), val and test metrics -- the numbers the log lines carry, for callers that compare runs."""
    model.train()
    graphed, capture_pending = None, bool(graph)
    early_stopping = EarlyStopping(patience=patience, verbose=True)
    topk = [int(k) for k in topk]
    # evaluation stays on the device when the model can hand the rank list over in HBM.  gene_ranklist returns 50 columns by
    # default, as the reference's does; a larger cut-off asks it for that many (the wide selection, up to MAX_TOPK), and one
    # beyond that fails here, before any epoch, instead of reporting "Recall@k" of a shorter list
    kmax = max(topk)
    if kmax > MAX_TOPK:
        raise ValueError(f"topk={topk}: the largest cut-off the rank lists serve is {MAX_TOPK}")
    on_device = getattr(model, "device", None) is not None and torch.device(model.device).type == "cuda"
    if on_device:
        val_data, test_data = EvalLists(val_data, model.device), EvalLists(test_data, model.device)
    spec = spec_of(model_name)
    if not spec.trains:
        # train_and_evaluate.py:531-552 (BSPM): nothing to train, no epochs -- rank once, evaluate both splits, return the test metrics
        model.eval()
        rank_list = _rank_list(model, kmax, on_device)
        val_metrics = evaluate(model, val_data, rank_list, topk)
        test_metrics = evaluate(model, test_data, rank_list, topk)
        _log_metrics('Validation Metrics:', val_metrics)
        _log_metrics('Test Metrics:', test_metrics)
        if history is not None:
            history.append({"epoch": 1, "loss": 0.0, "val": val_metrics, "test": test_metrics})
        return test_metrics
    for epoch in range(epochs):
        if spec.pre_epoch:
            model.pre_epoch_processing()
            if graphed is not None and getattr(model, "graph_generation", 0) != getattr(graphed, "_graph_generation", 0):
                graphed, capture_pending = None, bool(graph)     # the pruned graph was re-allocated: capture again
        if capture_pending:
            graphed, capture_pending = _capture_step(model, train_loader, optimizer, model_name), False
        loss = train(model, train_loader, optimizer, model_name, graphed)
        logging.info("Epoch {}, Loss: {:.5f}".format(epoch + 1, loss))

        model.eval()
        if hasattr(optimizer, "flush"):
            # lazily updated feature rows (optim.FusedAdam lazy_rows) are brought up to the current step at every epoch's end:
            # whoever reads a claimed table between epochs -- model.state_dict(), a checkpoint, a per-epoch kNN rebuild -- sees
            # current rows (one launch per claimed table; the rows' values are the eager ones bit for bit either way)
            optimizer.flush()
        rank_list = _rank_list(model, kmax, on_device)
        val_metrics = evaluate(model, val_data, rank_list, topk)
        test_metrics = evaluate(model, test_data, rank_list, topk)
        _log_metrics('Validation Metrics:', val_metrics)
        _log_metrics('Test Metrics:', test_metrics)
        if history is not None:
            history.append({"epoch": epoch + 1, "loss": loss, "val": val_metrics, "test": test_metrics})

        recall = test_metrics[max(topk)]['recall']
        early_stopping(recall, test_metrics)
        if early_stopping.early_stop:
            print("Early stopping")
            break

    if hasattr(optimizer, "flush"):
        optimizer.flush()          # lazily updated feature rows (optim.FusedAdam lazy_rows): current before anyone reads them
    best_metrics = early_stopping.best_metrics
    _log_metrics('Best Test Metrics:', best_metrics)
    return best_metrics
