"""The epoch loops that are not the generic `loss(*batch)` loop of train_and_evaluate.train: the in-launch replay path and the
models whose reference branch runs optimizers or phases of its own.  registry.MODELS names a model's loop in its `epoch` field;
the model loops share one signature, (model, train_loader, optimizer, ...optional extras)."""
import logging

import torch


def _cached_user_batches(model, key, train_loader, n, count=None):
    """The default user-id batches of a diffusion pass: dataload.DeviceUserBatches over n() ids at the train loader's batch size
    and seed -- `count` of them as a tuple, the m-th seeded seed + m -- made once and kept in model.__dict__[key] between epochs."""
    loaders = model.__dict__.get(key)
    if loaders is None:
        from .dataload import DeviceUserBatches
        seed = getattr(train_loader, "seed", 42)
        made = tuple(DeviceUserBatches(n(), train_loader.batch_size, model.device, seed + m) for m in range(count or 1))
        loaders = model.__dict__[key] = made if count else made[0]
    return loaders


def _train_epoch_in_launch(model, loader, optimizer, graphed):
    """One epoch with the batches drawn INSIDE the fused BPR forward (models with loss_drawn): the loader only lays
    down the epoch's permutation; every full batch is one argument-less graph replay, the short last batch (the
    reference's DataLoader keeps it, drop_last=False) one eager step on the same counters."""
    loader.begin_epoch()
    E, B = loader.edges.shape[0], loader.batch_size
    sum_loss = None
    if getattr(graphed, "fused", False):
        # optim.FusedLightGCNStep: several steps per replay, the per-batch losses summed on the device by the step itself
        graphed.loss_accum.zero_()
        # (a step with the light forward leaves the whole propagated table behind only when asked to: the epoch's last
        # step does, unless the short last batch below -- an ordinary forward -- comes after it)
        graphed.run(E // B, full_last=(E % B == 0))
        sum_loss = graphed.loss_accum[0].clone()
    else:
        for _ in range(E // B):
            d = graphed()
            sum_loss = d.clone() if sum_loss is None else sum_loss.add_(d)
    tail = E - (E // B) * B
    if tail:
        optimizer.zero_grad()
        loss = model.loss_drawn(loader.edges, tail, loader.seed, 0, step_dev=loader.step_dev, advance=True,
                                perm=loader.perm, perm_pos=loader.perm_pos)
        loss.backward()
        optimizer.step()
        d = loss.detach()
        sum_loss = d.clone() if sum_loss is None else sum_loss.add_(d)
    loader.global_step += len(loader)
    return float(sum_loss.item()) if sum_loss is not None else 0.0


def _train_epoch_mmssl(model, train_loader, optimizer):
    """reference train_and_evaluate.py:49-71: per batch a discriminator step (Adam, lr 3e-4, betas (0.5, 0.9)) and a generator step
    (AdamW over ALL of model.parameters(), the discriminator's included, at the run's learning rate); both optimizers are
    created anew every epoch there (their moments restart), the optimizer main() built is not used."""
    optim_D = torch.optim.Adam(model.D.parameters(), lr=3e-4, betas=(0.5, 0.9))
    optimizer_D = torch.optim.AdamW([{'params': model.parameters()}], lr=optimizer.param_groups[0]['lr'])
    sum_loss = None
    for idx, (users, pos_items, neg_items) in enumerate(train_loader):
        optim_D.zero_grad()
        loss_D = model.loss_D(users, pos_items, neg_items)
        loss_D.backward()
        optim_D.step()
        optimizer_D.zero_grad()
        batch_loss = model.loss(users, pos_items, neg_items, idx)
        batch_loss.backward(retain_graph=False)
        optimizer_D.step()
        d = (loss_D + batch_loss).detach()
        sum_loss = d.clone() if sum_loss is None else sum_loss.add_(d)
    return float(sum_loss.item()) if sum_loss is not None else 0.0


def _train_epoch_adagcl(model, train_loader, optimizer):
    """reference train_and_evaluate.py:72-97: three Adam optimizers created anew every epoch (their moments restart) -- `opt` over
    ALL parameters, one per generator (generator 2's with eps = 0.001) -- and per batch four losses: loss_1 and loss_2 each
    stepped by `opt`; bpr_reg_loss and gen_loss accumulate into one gradient, after which all three optimizers step, so the
    generators' parameters are stepped twice.  The optimizer main() built only gives the learning rate."""
    lr = optimizer.param_groups[0]['lr']
    opt = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=0)
    opt_gen_1 = torch.optim.Adam(model.generator_1.parameters(), lr=lr, weight_decay=0)
    opt_gen_2 = torch.optim.Adam(filter(lambda p: p.requires_grad, model.generator_2.parameters()), lr=lr, weight_decay=0, eps=0.001)
    sum_loss = None
    for users, pos_items, neg_items in train_loader:
        opt.zero_grad()
        opt_gen_1.zero_grad()
        opt_gen_2.zero_grad()
        loss_1, out1, out2 = model.loss_1(users, pos_items, neg_items)
        loss_1.backward()
        opt.step()
        opt.zero_grad()
        loss_2 = model.loss_2(users, pos_items, neg_items, out1, out2)
        loss_2.backward()
        opt.step()
        opt.zero_grad()
        bpr_reg_loss = model.bpr_reg_loss(users, pos_items, neg_items)
        bpr_reg_loss.backward()
        gen_loss = model.gen_loss(users, pos_items, neg_items)
        gen_loss.backward()
        opt.step()
        opt_gen_1.step()
        opt_gen_2.step()
        d = (loss_1 + loss_2 + bpr_reg_loss + gen_loss).detach()
        sum_loss = d.clone() if sum_loss is None else sum_loss.add_(d)
    return float(sum_loss.item()) if sum_loss is not None else 0.0


def _train_epoch_grade(model, train_loader, optimizer):
    """reference train_and_evaluate.py:259-284: four Adam optimizers created anew every epoch (their moments restart) -- `opt` over
    ALL parameters, one per generator -- and per batch three losses: loss_1 and bpr_reg_loss each stepped by `opt`, gen_loss
    stepped by the three generators' optimizers (the gradients it leaves on the embeddings are dropped by the next
    opt.zero_grad()).  The optimizer main() built only gives the learning rate."""
    lr = optimizer.param_groups[0]['lr']
    opt = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=0)
    opt_gen_1 = torch.optim.Adam(model.generator_1.parameters(), lr=lr, weight_decay=0)
    opt_gen_2 = torch.optim.Adam(model.generator_2.parameters(), lr=lr, weight_decay=0)
    opt_gen_3 = torch.optim.Adam(model.generator_3.parameters(), lr=lr, weight_decay=0)
    sum_loss = None
    for users, pos_items, neg_items in train_loader:
        opt.zero_grad()
        loss_1 = model.loss_1(users, pos_items, neg_items)
        loss_1.backward()
        opt.step()
        opt.zero_grad()
        bpr_reg_loss = model.bpr_reg_loss(users, pos_items, neg_items)
        bpr_reg_loss.backward()
        opt.step()
        opt_gen_1.zero_grad()
        opt_gen_2.zero_grad()
        opt_gen_3.zero_grad()
        gen_loss = model.gen_loss(users, pos_items, neg_items)
        gen_loss.backward()
        opt_gen_1.step()
        opt_gen_2.step()
        opt_gen_3.step()
        d = (loss_1 + gen_loss + bpr_reg_loss).detach()
        sum_loss = d.clone() if sum_loss is None else sum_loss.add_(d)
    return float(sum_loss.item()) if sum_loss is not None else 0.0


def _train_epoch_diffmm(model, train_loader, optimizer, diffusion_loader=None):
    """reference train_and_evaluate.py:140-244 in its three phases: (1) one pass of the diffusion loader, per batch a step of
    each denoiser under two Adam optimizers created anew every epoch (:142-145: their moments restart); (2) the two modal
    graphs rebuilt from the denoised rows; (3) the BPR steps over them.  The returned sum is the BPR losses', as there.
    diffusion_loader: user-id batches; by default a dataload.DeviceUserBatches at the train loader's batch size, kept on
    the model between epochs."""
    if diffusion_loader is None:
        diffusion_loader = _cached_user_batches(model, "_diffusion_loader", train_loader, lambda: model.num_user)
    lr = optimizer.param_groups[0]['lr']
    denoise_opt_image = torch.optim.Adam(model.denoise_model_image.parameters(), lr=lr, weight_decay=0)
    denoise_opt_text = torch.optim.Adam(model.denoise_model_text.parameters(), lr=lr, weight_decay=0)
    diff_sum = None
    for users in diffusion_loader:
        denoise_opt_image.zero_grad()
        denoise_opt_text.zero_grad()
        loss_image, loss_text = model.diffusion_step(users)
        loss = loss_image + loss_text
        loss.backward()
        denoise_opt_image.step()
        denoise_opt_text.step()
        d = loss.detach()
        diff_sum = d.clone() if diff_sum is None else diff_sum.add_(d)
    if diff_sum is not None:
        logging.info('Diffusion Loss (sum over %d steps) %.6f' % (len(diffusion_loader), float(diff_sum.item())))
    logging.info('Start to re-build UI matrix')
    image_adj, text_adj = model.rebuild_graphs(diffusion_loader)
    logging.info('UI matrix built!')
    sum_loss = None
    for users, pos_items, neg_items in train_loader:
        optimizer.zero_grad()
        loss = model.loss(users, pos_items, neg_items, image_adj, text_adj)
        loss.backward()
        optimizer.step()
        d = loss.detach()
        sum_loss = d.clone() if sum_loss is None else sum_loss.add_(d)
    return float(sum_loss.item()) if sum_loss is not None else 0.0


def _train_epoch_cfdiff(model, train_loader, optimizer, diffusion_loader=None):
    """reference train_and_evaluate.py:316-330: one pass over shuffled user batches, AdamW(weight_decay = 0) over CAM_AE created
    anew every epoch (its moments restart, as there).  A batch is its user ids: both hops' rows come from the history CSR
    (model.diffusion_step).  diffusion_loader: by default a dataload.DeviceUserBatches at the train loader's batch size, kept
    on the model between epochs.  The optimizer handed in is not read (main() builds none for this model)."""
    if diffusion_loader is None:
        diffusion_loader = _cached_user_batches(model, "_diffusion_loader", train_loader, lambda: model.num_user)
    optimizer = torch.optim.AdamW(model.CAM_AE.parameters(), lr=model.learning_rate, weight_decay=0)
    sum_loss = None
    for users in diffusion_loader:
        optimizer.zero_grad()
        loss = model.diffusion_step(users)
        loss.backward()
        optimizer.step()
        d = loss.detach()
        sum_loss = d.clone() if sum_loss is None else sum_loss.add_(d)
    return float(sum_loss.item()) if sum_loss is not None else 0.0


def _train_epoch_diffrec(model, train_loader, optimizer, diffusion_loader=None):
    """reference train_and_evaluate.py:304-315: one pass over shuffled user batches, AdamW(weight_decay = 0) over the denoiser
    created anew every epoch (its moments restart, as there).  A batch is its user ids: the noised rows come from the history
    CSR (model.diffusion_step).  diffusion_loader: by default a dataload.DeviceUserBatches at the train loader's batch size,
    kept on the model between epochs.  The optimizer handed in is not read (main() builds none for this model)."""
    if diffusion_loader is None:
        diffusion_loader = _cached_user_batches(model, "_diffusion_loader", train_loader, lambda: model.num_user)
    optimizer = torch.optim.AdamW(model.dnn.parameters(), lr=model.learning_rate, weight_decay=0)
    sum_loss = None
    for users in diffusion_loader:
        optimizer.zero_grad()
        loss = model.diffusion_step(users)
        loss.backward()
        optimizer.step()
        d = loss.detach()
        sum_loss = d.clone() if sum_loss is None else sum_loss.add_(d)
    return float(sum_loss.item()) if sum_loss is not None else 0.0


def _train_epoch_mhrec(model, train_loader, optimizer, diffusion_loaders=None, times=None):
    """reference train_and_evaluate.py:331-512 in its three phases: (1) one pass of the visual diffusion loader, then one of the
    textual, each denoiser under an Adam optimizer created anew every epoch (:333-336: their moments restart); (2) the two
    hypergraphs rebuilt from the denoised rows' top-k; (3) the BPR steps over them.  The returned sum is the BPR losses', as
    there.  diffusion_loaders: a pair of iterables of input-hyperedge index batches; by default two dataload.DeviceUserBatches
    over the interactions at the train loader's batch size, kept on the model between epochs.  times (optional dict): receives
    the three phases' wall times in seconds (each ends with a device synchronisation)."""
    import time
    if diffusion_loaders is None:
        diffusion_loaders = _cached_user_batches(model, "_diffusion_loaders", train_loader,
                                                 lambda: model.diffusion_tables()[0].shape[0], count=2)

    def mark(name, t0):
        if times is not None:
            torch.cuda.synchronize()
            times[name] = time.perf_counter() - t0
        return time.perf_counter()
    t0 = time.perf_counter()
    lr = optimizer.param_groups[0]['lr']
    opts = (torch.optim.Adam(model.denoise_model_image.parameters(), lr=lr, weight_decay=0),
            torch.optim.Adam(model.denoise_model_text.parameters(), lr=lr, weight_decay=0))
    for m, (opt, loader) in enumerate(zip(opts, diffusion_loaders)):
        diff_sum = None
        for batch in loader:
            opt.zero_grad()
            loss = model.diffusion_step(batch, m)
            loss.backward()
            opt.step()
            d = loss.detach()
            diff_sum = d.clone() if diff_sum is None else diff_sum.add_(d)
        if diff_sum is not None:
            logging.info('%s hyperedges: Diffusion Loss (sum over %d steps) %.6f' % (("visual", "textual")[m], len(loader), float(diff_sum.item())))
    t0 = mark("diffusion", t0)
    logging.info('Start to re-build hypergraph matrix')
    G_visual, G_textual = model.rebuild_hypergraphs(*diffusion_loaders)
    logging.info('hypergraph matrix built!')
    t0 = mark("rebuild", t0)
    sum_loss = None
    for users, pos_items, neg_items in train_loader:
        optimizer.zero_grad()
        loss = model.loss(users, pos_items, neg_items, G_visual, G_textual)
        loss.backward()
        optimizer.step()
        d = loss.detach()
        sum_loss = d.clone() if sum_loss is None else sum_loss.add_(d)
    out = float(sum_loss.item()) if sum_loss is not None else 0.0
    mark("bpr", t0)
    return out
