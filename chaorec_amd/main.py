"""Entry point: `python -m chaorec_amd.main --Model LightGCN --data_path sports` (reference main.py:73-442).

Same flow: parse flags, seed, load data, build the sampler, cartesian product over the model's YAML grid,
construct the model, Adam, train_and_evaluate, keep the best combination by Recall@20.  Out of scope and
dropped: the 51 other constructors and the dense U x I DiffusionData the reference builds for every model
(main.py:202; 1.76 GB for sports)."""
import logging
import os
from itertools import product

import torch
from torch.utils.data import DataLoader

from . import dataload
from .Model import (AdaGCL, BM3, BPRMF, BSPM, CF_Diff, COHESION, DCCF, DGCF, DDRec, DHCF, DRAGON, DualGNN, DualVAE, FKAN_GCF, FREEDOM, GRCN, GUME, Grade, GraphAug, HCCF, LATTICE, LGMRec, LightGCL, LayerGCN, LightGCN, LightGT, MCLN, MENTOR, MGAT, MGCL, MGCN, MHRec, MICRO, MMGCN, MMSSL, MVGAE, MacridVAE, DiffMM, MultVAE, NCL, NGCF, MMGCL, POWERec, SelfCF, SGL, SimGCL, SLMRec,
                    SMORE, VBPR, VGCL, XSimGCL)
from .arg_parser import load_yaml_config, parse_args
from .train_and_evaluate import train_and_evaluate
from .optim import FusedAdam
from .utils import get_local_time, gpu, setup_seed


def setup_logging(args):
    log_dir = "log"
    os.makedirs(log_dir, exist_ok=True)
    log_filename = os.path.join(log_dir, f"{args.Model}_{args.data_path}").replace("\\", "/") + ".log"
    fmt = logging.Formatter('%(asctime)s %(levelname)s %(message)s', '%a %d %b %Y %H:%M:%S')
    logger = logging.getLogger()
    logger.setLevel(logging.INFO)
    for h in (logging.StreamHandler(), logging.FileHandler(log_filename, mode='w')):
        h.setLevel(logging.INFO)
        h.setFormatter(fmt)
        logger.addHandler(h)


def build_model(args, num_user, num_item, train_data, user_item_dict, v_feat, t_feat, device):
    """The rows of the reference's constructor table on the hot path (main.py:261-263, :267-270, :287-289, :316-317, :323-324)."""
    dim_E, aggr_mode = args.dim_E, args.aggr_mode
    table = {
        'MMGCN': lambda: MMGCN(num_user, num_item, train_data, user_item_dict, v_feat, t_feat, dim_E, args.reg_weight,
                               aggr_mode, 'False', True, device),
        'LightGCN': lambda: LightGCN(num_user, num_item, train_data, user_item_dict, dim_E, args.reg_weight,
                                     args.n_layers, aggr_mode, device),
        'NGCF': lambda: NGCF(num_user, num_item, train_data, user_item_dict, dim_E, args.reg_weight, args.dropout,
                             args.n_layers, aggr_mode, device),
        'FREEDOM': lambda: FREEDOM(num_user, num_item, train_data, user_item_dict, v_feat, t_feat, dim_E,
                                   args.feature_embed, args.reg_weight, args.dropout, args.n_layers, args.mm_layers,
                                   args.ii_topk, args.lambda_coeff, device),
        'LayerGCN': lambda: LayerGCN(num_user, num_item, train_data, user_item_dict, dim_E, args.reg_weight,
                                     args.n_layers, args.dropout, device),
        'MGCN': lambda: MGCN(num_user, num_item, train_data, user_item_dict, v_feat, t_feat, dim_E, args.reg_weight,
                             args.n_layers, aggr_mode, args.ssl_temp, args.ssl_alpha, device),
        'BPR': lambda: BPRMF(num_user, num_item, user_item_dict, dim_E, args.reg_weight, device),
        'VBPR': lambda: VBPR(num_user, num_item, user_item_dict, v_feat, dim_E, args.feature_embed, args.reg_weight,
                             device),
        # three more members of the torch.sparse.mm family, through the adapter alone (main.py:305-306, :335-336, :344-345)
        'NCL': lambda: NCL(num_user, num_item, train_data, user_item_dict, dim_E, args.reg_weight, args.n_layers, aggr_mode,
                           args.ssl_temp, args.ssl_alpha, device),
        'SimGCL': lambda: SimGCL(num_user, num_item, train_data, user_item_dict, dim_E, args.reg_weight, args.n_layers,
                                 args.ssl_temp, args.ssl_alpha, device),
        'XSimGCL': lambda: XSimGCL(num_user, num_item, train_data, user_item_dict, dim_E, args.reg_weight, args.n_layers,
                                   args.ssl_temp, args.ssl_alpha, device),
        'SLMRec': lambda: SLMRec(num_user, num_item, train_data, user_item_dict, v_feat, t_feat, dim_E, args.n_layers,
                                 args.ssl_temp, args.ssl_alpha, device),
        'SelfCF': lambda: SelfCF(num_user, num_item, train_data, user_item_dict, dim_E, args.reg_weight, args.n_layers,
                                 args.dropout, device),
        # the one reader of the sampler's second negative (main.py:354-355, dataload.py:81-84)
        'MCLN': lambda: MCLN(num_user, num_item, train_data, user_item_dict, v_feat, t_feat, dim_E, args.reg_weight,
                             args.n_layers, args.n_mca, device),
        # round 5: four more members (main.py:318-320, :342-343, :358-359, :377-378)
        'POWERec': lambda: POWERec(num_user, num_item, train_data, user_item_dict, v_feat, t_feat, dim_E, args.reg_weight,
                                   args.n_layers, int(args.prompt_num), args.neg_weight, args.dropout, device),
        'LGMRec': lambda: LGMRec(num_user, num_item, train_data, user_item_dict, v_feat, t_feat, dim_E, args.reg_weight,
                                 args.n_layers, args.ssl_alpha, device),
        'DHCF': lambda: DHCF(num_user, num_item, train_data, user_item_dict, dim_E, args.reg_weight, args.n_layers,
                             args.dropout, device),
        'FKAN_GCF': lambda: FKAN_GCF(num_user, num_item, train_data, user_item_dict, dim_E, args.reg_weight, args.n_layers,
                                     args.node_dropout, args.message_dropout, args.grid_size, device),
        'LightGT': lambda: LightGT(num_user, num_item, train_data, user_item_dict, v_feat, t_feat, dim_E, args.reg_weight,
                                   args.n_layers, device),
        'MMGCL': lambda: MMGCL(num_user, num_item, train_data, user_item_dict, v_feat, t_feat, dim_E, args.reg_weight,
                               args.n_layers, args.ssl_alpha, args.ssl_temp, args.dropout, device),
        # (main.py:282-283, :314-315)
        'BM3': lambda: BM3(num_user, num_item, train_data, user_item_dict, v_feat, t_feat, dim_E, args.feature_embed, args.reg_weight,
                           args.dropout, args.n_layers, args.cl_weight, aggr_mode, device),
        'MGCL': lambda: MGCL(num_user, num_item, train_data, user_item_dict, v_feat, t_feat, dim_E, args.reg_weight, args.n_layers,
                             aggr_mode, args.ssl_temp, args.ssl_alpha, device),
        # (main.py:302-303)
        'SGL': lambda: SGL(num_user, num_item, train_data, user_item_dict, dim_E, args.reg_weight, args.n_layers, aggr_mode,
                           args.ssl_temp, args.ssl_alpha, device),
        # (main.py:309-313)
        'LightGCL': lambda: LightGCL(num_user, num_item, train_data, user_item_dict, dim_E, args.reg_weight, args.n_layers, aggr_mode,
                                     args.ssl_alpha, args.ssl_temp, device),
        'HCCF': lambda: HCCF(num_user, num_item, train_data, user_item_dict, dim_E, args.reg_weight, args.n_layers, aggr_mode,
                             args.ssl_alpha, args.ssl_temp, args.keepRate, args.leaky, args.mult, device),
        # (main.py:346-348)
        'MENTOR': lambda: MENTOR(num_user, num_item, train_data, user_item_dict, v_feat, t_feat, dim_E, args.mm_layers, args.reg_weight,
                                 args.ssl_temp, args.dropout, args.align_weight, args.mask_weight_g, args.mask_weight_f, device),
        # (main.py:276-279)
        'LATTICE': lambda: LATTICE(num_user, num_item, train_data, user_item_dict, v_feat, t_feat, dim_E, args.feature_embed, args.reg_weight,
                                   args.n_layers, args.mm_layers, args.ii_topk, aggr_mode, args.lambda_coeff, device),
        # (main.py:294-296)
        'MICRO': lambda: MICRO(num_user, num_item, train_data, user_item_dict, v_feat, t_feat, dim_E, args.n_layers, args.reg_weight,
                               args.ii_topk, args.mm_layers, args.ssl_temp, args.lambda_coeff, args.ssl_alpha, aggr_mode, device),
        # (main.py:325-326)
        'DCCF': lambda: DCCF(num_user, num_item, train_data, user_item_dict, dim_E, args.reg_weight, args.n_layers, args.ssl_temp,
                             args.ssl_alpha, args.n_intents, args.cen_reg, device),
        # (main.py:299-301)
        'DDRec': lambda: DDRec(num_user, num_item, train_data, user_item_dict, v_feat, t_feat, dim_E, args.feature_embed,
                               args.reg_weight, args.n_layers, args.ssl_temp, args.ssl_alpha, args.threshold, aggr_mode, device),
        # (main.py:292-293)
        'MGAT': lambda: MGAT(num_user, num_item, train_data, user_item_dict, v_feat, t_feat, dim_E, args.reg_weight, device),
        # (main.py:271-273)
        'GRCN': lambda: GRCN(num_user, num_item, train_data, user_item_dict, v_feat, t_feat, dim_E, args.feature_embed, args.reg_weight,
                             args.dropout, args.n_iterations, aggr_mode, device),
        # (main.py:331-332)
        'MMSSL': lambda: MMSSL(num_user, num_item, train_data, user_item_dict, v_feat, t_feat, dim_E, args.reg_weight, args.ssl_alpha,
                               args.ssl_temp, args.G_rate, args.mm_layers, device),
        # (main.py:333-334)
        'VGCL': lambda: VGCL(num_user, num_item, train_data, user_item_dict, dim_E, args.reg_weight, args.n_layers,
                             args.ssl_temp, args.ssl_alpha, device),
        # (main.py:379-380)
        'GUME': lambda: GUME(num_user, num_item, train_data, user_item_dict, v_feat, t_feat, dim_E, args.n_layers,
                             args.n_ui_layers, args.um_loss, args.vt_loss, args.data_path, device),
        # (main.py:274-275)
        'DGCF': lambda: DGCF(num_user, num_item, train_data, user_item_dict, dim_E, args.reg_weight, args.corDecay,
                             args.n_factors, args.n_iterations, args.n_layers, aggr_mode, device),
        # (main.py:304) the first of the autoencoder family: kernels of its own, csrc/multvae.hip
        'MultVAE': lambda: MultVAE(num_user, num_item, train_data, user_item_dict, dim_E, args.reg_weight, device),
        # (main.py:307) its K-prototype mixture likelihood on the same machinery, csrc/macridvae.hip
        'MacridVAE': lambda: MacridVAE(num_user, num_item, train_data, user_item_dict, dim_E, args.reg_weight, device),
        # (main.py:329) both sides' aspect encoders and the Poisson likelihood on kernels of their own, csrc/dualvae.hip
        'DualVAE': lambda: DualVAE(num_user, num_item, train_data, user_item_dict, dim_E, args.reg_weight, args.ssl_alpha,
                                   device),
        'SMORE': lambda: SMORE(num_user, num_item, train_data, user_item_dict, v_feat, t_feat, dim_E, args.reg_weight,
                               args.n_ui_layers, args.ii_topk, args.dropout, args.data_path, device),
        # (main.py:284) the user-user co-occurrence graph built, sampled and aggregated on the device, csrc/usergraph.hip
        'DRAGON': lambda: DRAGON(num_user, num_item, train_data, user_item_dict, v_feat, t_feat, dim_E, args.feature_embed,
                                 args.reg_weight, args.n_layers, args.ii_topk, args.uu_topk, args.lambda_coeff, aggr_mode, device),
        # (main.py:280) the model DRAGON derives from: the same graph, its aggregation fused with the modality mix and the item rows
        'DualGNN': lambda: DualGNN(num_user, num_item, train_data, user_item_dict, v_feat, t_feat, dim_E, args.feature_embed,
                                   args.reg_weight, args.uu_topk, aggr_mode, device),
        # (main.py:381-383) the reference's default model: three modality tables side by side over the same user graph
        # (k = 40 hard-coded), a chunked backward; mm_image_weight comes from Model_YAML/COHESION.yaml
        'COHESION': lambda: COHESION(num_user, num_item, train_data, user_item_dict, v_feat, t_feat, dim_E, args.reg_weight,
                                     args.dropout, args.n_layers, args.mm_layers, args.ii_topk, args.mm_image_weight, device),
        # (main.py:321-322) three modality GCNs into a product of experts: the conv epilogue and the PoE / KL / BPR tail are
        # one launch and one autograd node, csrc/mvgae.hip
        'MVGAE': lambda: MVGAE(num_user, num_item, train_data, user_item_dict, v_feat, t_feat, dim_E, args.reg_weight,
                               args.n_layers, device),
        # (main.py:360-362) the graph half through the adapter; the diffusion half -- noised history rows, the denoiser's output
        # layer with both losses and its gradient in one pass -- on kernels of its own, csrc/diffmm.hip
        'DiffMM': lambda: DiffMM(num_user, num_item, train_data, user_item_dict, v_feat, t_feat, dim_E, args.reg_weight,
                                 args.n_layers, args.ssl_alpha, args.ssl_temp, args.ris_lambda, args.e_loss, args.rebuild_k,
                                 device),
        # (main.py:327-328) two learned view generators over one fixed structure: the edge gate from two per-node scores and
        # the per-edge keep MLP on the f32 MFMA pipe, csrc/adagcl.hip; three optimizers per batch (train_and_evaluate.py:72-97)
        # (main.py:365-367) AdaGCL's vgae generator three times over -- ID, visual, textual -- on a FREEDOM-style item graph: the
        # three views of a step from one fused node (the MLP per undirected pair, weighted row sums, values), csrc/grade.hip;
        # four optimizers per batch (train_and_evaluate.py:259-284)
        'Grade': lambda: Grade(num_user, num_item, train_data, user_item_dict, v_feat, t_feat, dim_E, args.reg_weight,
                               args.n_layers, args.ssl_temp, args.ssl_alpha, args.ssl_temp2, args.noise_alpha, device),
        'AdaGCL': lambda: AdaGCL(num_user, num_item, train_data, user_item_dict, dim_E, args.reg_weight, args.n_layers,
                                 args.ssl_temp, args.ssl_alpha, device),
        # (main.py:339-341) a learned view sampler over the fixed structure plus 100 000 random entries per step: the per-edge
        # sampler and the contrastive terms' whole-table log-sum-exp on kernels of their own, csrc/graphaug.hip
        'GraphAug': lambda: GraphAug(num_user, num_item, train_data, user_item_dict, dim_E, args.reg_weight, args.n_layers,
                                     args.ssl_temp, args.ssl_alpha, device),
        # (main.py:374-376) two hypergraphs rebuilt every epoch from denoised hyperedge rows; the hypergraph attention layer with
        # its residual and dropout is one autograd node, csrc/mhrec.hip; three phases per epoch (train_and_evaluate.py:331-512)
        'MHRec': lambda: MHRec(num_user, num_item, train_data, user_item_dict, v_feat, t_feat, dim_E, args.reg_weight,
                               args.ii_topk, args.uu_topk, args.num_hypernodes, args.n_layers, args.h_layers, args.ssl_temp,
                               args.ssl_alpha, args.beta1, args.beta2, device),
        # (main.py:368-369) the one model that trains nothing: an item-item filter built once, every user's history row blurred,
        # sharpened and ranked, csrc/bspm.hip.  The reference passes args.K_s where T_b belongs; neither is read, T_b it is here
        'BSPM': lambda: BSPM(num_user, num_item, train_data, user_item_dict, args.K_s, args.T_s, args.K_b, args.T_b,
                             args.idl_beta, device),
        # (main.py:372-373) the cross-attention denoiser: its rows come from the history CSR, its attention is csrc/cfdiff.hip
        'CF_Diff': lambda: CF_Diff(num_user, num_item, user_item_dict, args.noise_scale, args.noise_min, args.noise_max,
                                   args.steps, args.learning_rate, device, seed=args.seed),
    }
    if args.Model == 'MHRec':      # Model/MHRec.py:578, :604-612 read user_graph_dict.npy and the hyperedge files there
        MHRec.data_dir = os.path.join(args.data_root, args.data_path)
    if args.Model == 'COHESION':   # Model/COHESION.py:96-99 reads the same file
        COHESION.user_graph_path = os.path.join(args.data_root, args.data_path, 'user_graph_dict.npy')
    if args.Model == 'DualGNN':    # Model/DualGNN.py:166-170 reads the same file
        DualGNN.user_graph_path = os.path.join(args.data_root, args.data_path, 'user_graph_dict.npy')
    if args.Model == 'DRAGON':     # Model/DRAGON.py:168-171 reads this file; where it is missing the graph is built on the device
        DRAGON.user_graph_path = os.path.join(args.data_root, args.data_path, 'user_graph_dict.npy')
    if args.Model not in table:
        raise SystemExit(f"--Model {args.Model}: only {sorted(table)} are on the MI355X hot path")
    return table[args.Model]()


def main(argv=None):
    args = parse_args(argv)
    setup_logging(args)
    logging.info('============Arguments==============')
    for arg, value in vars(args).items():
        logging.info('%s: %s', arg, value)
    logging.info('local time：%s', get_local_time())
    setup_seed(args.seed)
    device = gpu()
    if device.type != "cuda":
        raise SystemExit("chaorec_amd runs on the MI355X only: no GPU visible")
    config = load_yaml_config(args.Model)
    needs_feat = args.Model in ("MMGCN", "FREEDOM", "MGCN", "VBPR", "SLMRec", "MCLN", "POWERec", "LGMRec", "SMORE", "MMGCL", "LightGT", "GUME", "DDRec", "MICRO", "MENTOR", "BM3", "MGCL", "LATTICE", "MMSSL", "GRCN", "MGAT", "DRAGON", "DualGNN", "COHESION", "MVGAE", "DiffMM", "Grade", "MHRec")
    train_data, val_data, test_data, user_item_dict, num_user, num_item, v_feat, t_feat = dataload.data_load(
        args.data_path, has_v=needs_feat, has_t=needs_feat, data_root=args.data_root, synthetic=args.synthetic)
    if args.host_sampler:
        ds = dataload.TrainingDataset(num_user, num_item, user_item_dict, train_data, args.Model)
        train_loader = DataLoader(ds, args.batch_size, shuffle=True, num_workers=args.num_workers)
    else:
        train_loader = dataload.DeviceBatchSampler(num_user, num_item, user_item_dict, train_data, args.batch_size,
                                                   device, args.Model, args.seed)
    args.num_user, args.num_item = num_user, num_item

    combinators = list(product(*[config[p] for p in config['hyper_parameters']]))
    best_performance, best_params, best_metrics = None, None, None
    for idx, combo in enumerate(combinators):
        hyper = dict(zip(config['hyper_parameters'], combo))
        logging.info('========={}/{}: Parameters:{}========='.format(idx + 1, len(combinators), hyper))
        for key, value in hyper.items():
            setattr(args, key, value)
        model = build_model(args, num_user, num_item, train_data, user_item_dict, v_feat, t_feat, device)
        model.to(device)
        # reference: torch.optim.Adam (main.py:397); same update, one fused launch per tensor
        # (BSPM has no parameter: no optimizer, as its branch of train_and_evaluate never steps one; CF_Diff's epoch creates its
        # own AdamW over CAM_AE, train_and_evaluate.py:317)
        optimizer = None if args.Model in ('BSPM', 'CF_Diff') else FusedAdam([{'params': model.parameters(), 'lr': args.learning_rate}])
        current = train_and_evaluate(model, train_loader, val_data, test_data, optimizer, args.num_epoch,
                                     model_name=args.Model, topk=args.topk, patience=args.patience,
                                     graph=not args.no_graph)
        recall = current[20]['recall'] if 20 in current else current[max(current)]['recall']
        if best_performance is None or recall > best_performance:
            best_performance, best_params, best_metrics = recall, hyper.copy(), current
    logging.info("Best performance: {:.5f}".format(best_performance))
    logging.info("Best parameters: {}".format(best_params))
    logging.info("Best metrics:")
    for k, m in best_metrics.items():
        logging.info(f"{k}: {' | '.join(f'{name}: {value:.5f}' for name, value in m.items())}")
    return best_metrics


if __name__ == '__main__':
    main()
