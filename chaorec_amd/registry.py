"""The one table of models: what main, the training loop and the tools need to know about a --Model name.

A row is the reference's constructor row (main.py:261-383; the arguments as there) plus the traits in which the model departs
from the generic case -- a (users, pos, neg) batch, one `loss(*batch)` step per batch under main's FusedAdam, captured where
the loader and optimizer allow it.  A plain model's row is its constructor and nothing else."""
import os
from collections import namedtuple
from dataclasses import dataclass
from typing import Callable, Optional

from . import Model as M, epochs

# what a constructor row reads besides the flags; rows spell the common head as *d[:4] (num_user .. user_item_dict) or *d[:6]
ModelData = namedtuple("ModelData", "num_user num_item train_data user_item_dict v_feat t_feat device")


@dataclass(frozen=True)
class ModelSpec:
    build: Optional[Callable]                 # (args, d: ModelData) -> the model
    features: bool = False                    # reads v_feat / t_feat: main loads them
    batch: str = "triple"                     # what the samplers hand it: "triple" | "pairs" (MMGCN's two [2B] tensors) | "second_negative" | "sequences"
    pre_epoch: bool = False                   # pre_epoch_processing() before every epoch (reference train_and_evaluate.py:555)
    before_step: Optional[Callable] = None    # called on the model before every eager step
    build_first: bool = False                 # loss(..., build_item_graph=<first batch of the epoch>) (reference :96-103)
    capture: bool = True                      # the step may be captured into a hipGraph; a row says why not
    epoch: Optional[Callable] = None          # a loop of its own from epochs.py, (model, train_loader, optimizer) -> summed loss
    trains: bool = True                       # False: nothing to train -- rank once, evaluate both splits
    main_optimizer: bool = True               # main builds a FusedAdam over model.parameters()


def _at(cls, attr, *path):
    """Point the class attribute a model reads its side files from at os.path.join(*path); returns the class."""
    setattr(cls, attr, os.path.join(*path))
    return cls


# (capture: SimGCL / XSimGCL / SLMRec draw only with rand_like on the device generator, which a captured step advances per replay:
# they are captured -- round 5: 2 x the eager epoch rate at baby size, tools/capture_family_probe.py)
MODELS = {
    'MMGCN': ModelSpec(lambda a, d: M.MMGCN(*d[:6], a.dim_E, a.reg_weight, a.aggr_mode, 'False', True, d.device), features=True, batch="pairs"),
    'LightGCN': ModelSpec(lambda a, d: M.LightGCN(*d[:4], a.dim_E, a.reg_weight, a.n_layers, a.aggr_mode, d.device)),
    'NGCF': ModelSpec(lambda a, d: M.NGCF(*d[:4], a.dim_E, a.reg_weight, a.dropout, a.n_layers, a.aggr_mode, d.device)),
    'FREEDOM': ModelSpec(lambda a, d: M.FREEDOM(*d[:6], a.dim_E, a.feature_embed, a.reg_weight, a.dropout, a.n_layers, a.mm_layers, a.ii_topk,
                                               a.lambda_coeff, d.device), features=True, pre_epoch=True),
    'LayerGCN': ModelSpec(lambda a, d: M.LayerGCN(*d[:4], a.dim_E, a.reg_weight, a.n_layers, a.dropout, d.device), pre_epoch=True),
    'MGCN': ModelSpec(lambda a, d: M.MGCN(*d[:6], a.dim_E, a.reg_weight, a.n_layers, a.aggr_mode, a.ssl_temp, a.ssl_alpha, d.device), features=True),
    'BPR': ModelSpec(lambda a, d: M.BPRMF(d.num_user, d.num_item, d.user_item_dict, a.dim_E, a.reg_weight, d.device)),
    'VBPR': ModelSpec(lambda a, d: M.VBPR(d.num_user, d.num_item, d.user_item_dict, d.v_feat, a.dim_E, a.feature_embed, a.reg_weight, d.device), features=True),
    # three more members of the torch.sparse.mm family, through the adapter alone (main.py:305-306, :335-336, :344-345)
    # NCL clusters its embeddings before EVERY batch (train_and_evaluate.py:107-114): k-means with host decisions, eager
    'NCL': ModelSpec(lambda a, d: M.NCL(*d[:4], a.dim_E, a.reg_weight, a.n_layers, a.aggr_mode, a.ssl_temp, a.ssl_alpha, d.device),
                     before_step=lambda m: m.e_step(), capture=False),
    'SimGCL': ModelSpec(lambda a, d: M.SimGCL(*d[:4], a.dim_E, a.reg_weight, a.n_layers, a.ssl_temp, a.ssl_alpha, d.device)),
    'XSimGCL': ModelSpec(lambda a, d: M.XSimGCL(*d[:4], a.dim_E, a.reg_weight, a.n_layers, a.ssl_temp, a.ssl_alpha, d.device)),
    'SLMRec': ModelSpec(lambda a, d: M.SLMRec(*d[:6], a.dim_E, a.n_layers, a.ssl_temp, a.ssl_alpha, d.device), features=True),
    # not captured: its dropout rate is np.random.random() per step (Model/SelfCF.py:55), a capture would freeze it
    'SelfCF': ModelSpec(lambda a, d: M.SelfCF(*d[:4], a.dim_E, a.reg_weight, a.n_layers, a.dropout, d.device), capture=False),
    # the one reader of the sampler's second negative (main.py:354-355, dataload.py:81-84)
    'MCLN': ModelSpec(lambda a, d: M.MCLN(*d[:6], a.dim_E, a.reg_weight, a.n_layers, a.n_mca, d.device), features=True, batch="second_negative"),
    # round 5: four more members (main.py:318-320, :342-343, :358-359, :377-378)
    'POWERec': ModelSpec(lambda a, d: M.POWERec(*d[:6], a.dim_E, a.reg_weight, a.n_layers, int(a.prompt_num), a.neg_weight, a.dropout, d.device), features=True, pre_epoch=True),
    'LGMRec': ModelSpec(lambda a, d: M.LGMRec(*d[:6], a.dim_E, a.reg_weight, a.n_layers, a.ssl_alpha, d.device), features=True),
    'DHCF': ModelSpec(lambda a, d: M.DHCF(*d[:4], a.dim_E, a.reg_weight, a.n_layers, a.dropout, d.device)),
    'FKAN_GCF': ModelSpec(lambda a, d: M.FKAN_GCF(*d[:4], a.dim_E, a.reg_weight, a.n_layers, a.node_dropout, a.message_dropout, a.grid_size, d.device)),
    # not captured: its batches carry history sequences built on the host
    'LightGT': ModelSpec(lambda a, d: M.LightGT(*d[:6], a.dim_E, a.reg_weight, a.n_layers, d.device), features=True, batch="sequences", capture=False),
    # not captured: hipErrorStreamCaptureUnsupported inside the per-step view construction
    'MMGCL': ModelSpec(lambda a, d: M.MMGCL(*d[:6], a.dim_E, a.reg_weight, a.n_layers, a.ssl_alpha, a.ssl_temp, a.dropout, d.device), features=True, capture=False),
    # (main.py:282-283, :314-315)
    'BM3': ModelSpec(lambda a, d: M.BM3(*d[:6], a.dim_E, a.feature_embed, a.reg_weight, a.dropout, a.n_layers, a.cl_weight, a.aggr_mode, d.device), features=True),
    'MGCL': ModelSpec(lambda a, d: M.MGCL(*d[:6], a.dim_E, a.reg_weight, a.n_layers, a.aggr_mode, a.ssl_temp, a.ssl_alpha, d.device), features=True),
    # (main.py:302-303) not captured: hipErrorStreamCaptureUnsupported inside the per-step view construction
    'SGL': ModelSpec(lambda a, d: M.SGL(*d[:4], a.dim_E, a.reg_weight, a.n_layers, a.aggr_mode, a.ssl_temp, a.ssl_alpha, d.device), capture=False),
    # (main.py:309-313)
    'LightGCL': ModelSpec(lambda a, d: M.LightGCL(*d[:4], a.dim_E, a.reg_weight, a.n_layers, a.aggr_mode, a.ssl_alpha, a.ssl_temp, d.device)),
    'HCCF': ModelSpec(lambda a, d: M.HCCF(*d[:4], a.dim_E, a.reg_weight, a.n_layers, a.aggr_mode, a.ssl_alpha, a.ssl_temp, a.keepRate, a.leaky, a.mult, d.device)),
    # (main.py:346-348)
    'MENTOR': ModelSpec(lambda a, d: M.MENTOR(*d[:6], a.dim_E, a.mm_layers, a.reg_weight, a.ssl_temp, a.dropout, a.align_weight, a.mask_weight_g,
                                             a.mask_weight_f, d.device), features=True),
    # (main.py:276-279) the first batch of an epoch rebuilds the item graphs: the structure changes, not captured
    'LATTICE': ModelSpec(lambda a, d: M.LATTICE(*d[:6], a.dim_E, a.feature_embed, a.reg_weight, a.n_layers, a.mm_layers, a.ii_topk, a.aggr_mode,
                                               a.lambda_coeff, d.device), features=True, build_first=True, capture=False),
    # (main.py:294-296) as LATTICE
    'MICRO': ModelSpec(lambda a, d: M.MICRO(*d[:6], a.dim_E, a.n_layers, a.reg_weight, a.ii_topk, a.mm_layers, a.ssl_temp, a.lambda_coeff, a.ssl_alpha,
                                           a.aggr_mode, d.device), features=True, build_first=True, capture=False),
    # (main.py:325-326)
    'DCCF': ModelSpec(lambda a, d: M.DCCF(*d[:4], a.dim_E, a.reg_weight, a.n_layers, a.ssl_temp, a.ssl_alpha, a.n_intents, a.cen_reg, d.device)),
    # (main.py:299-301)
    'DDRec': ModelSpec(lambda a, d: M.DDRec(*d[:6], a.dim_E, a.feature_embed, a.reg_weight, a.n_layers, a.ssl_temp, a.ssl_alpha, a.threshold,
                                           a.aggr_mode, d.device), features=True),
    # (main.py:292-293)
    'MGAT': ModelSpec(lambda a, d: M.MGAT(*d[:6], a.dim_E, a.reg_weight, d.device), features=True),
    # (main.py:271-273)
    'GRCN': ModelSpec(lambda a, d: M.GRCN(*d[:6], a.dim_E, a.feature_embed, a.reg_weight, a.dropout, a.n_iterations, a.aggr_mode, d.device), features=True, batch="pairs"),
    # (main.py:331-332) not captured: several optimizers per batch, its own loop
    'MMSSL': ModelSpec(lambda a, d: M.MMSSL(*d[:6], a.dim_E, a.reg_weight, a.ssl_alpha, a.ssl_temp, a.G_rate, a.mm_layers, d.device),
                       features=True, capture=False, epoch=epochs._train_epoch_mmssl),
    # (main.py:333-334) VGCL clusters the noised view of THIS forward (train_and_evaluate.py:116-125; its loss() runs none), eager as NCL
    'VGCL': ModelSpec(lambda a, d: M.VGCL(*d[:4], a.dim_E, a.reg_weight, a.n_layers, a.ssl_temp, a.ssl_alpha, d.device),
                      before_step=lambda m: (m.forward(), m.e_step()), capture=False),
    # (main.py:379-380)
    'GUME': ModelSpec(lambda a, d: M.GUME(*d[:6], a.dim_E, a.n_layers, a.n_ui_layers, a.um_loss, a.vt_loss, a.data_path, d.device), features=True),
    # (main.py:274-275)
    'DGCF': ModelSpec(lambda a, d: M.DGCF(*d[:4], a.dim_E, a.reg_weight, a.corDecay, a.n_factors, a.n_iterations, a.n_layers, a.aggr_mode, d.device)),
    # (main.py:304) the first of the autoencoder family: kernels of its own, csrc/multvae.hip
    'MultVAE': ModelSpec(lambda a, d: M.MultVAE(*d[:4], a.dim_E, a.reg_weight, d.device)),
    # (main.py:307) its K-prototype mixture likelihood on the same machinery, csrc/macridvae.hip
    'MacridVAE': ModelSpec(lambda a, d: M.MacridVAE(*d[:4], a.dim_E, a.reg_weight, d.device)),
    # (main.py:329) both sides' aspect encoders and the Poisson likelihood on kernels of their own, csrc/dualvae.hip
    'DualVAE': ModelSpec(lambda a, d: M.DualVAE(*d[:4], a.dim_E, a.reg_weight, a.ssl_alpha, d.device)),
    'SMORE': ModelSpec(lambda a, d: M.SMORE(*d[:6], a.dim_E, a.reg_weight, a.n_ui_layers, a.ii_topk, a.dropout, a.data_path, d.device), features=True),
    # (main.py:284) the user-user co-occurrence graph built, sampled and aggregated on the device, csrc/usergraph.hip
    # (Model/DRAGON.py:168-171, DualGNN.py:166-170 and COHESION.py:96-99 read user_graph_dict.npy; DRAGON builds the graph where it is missing)
    'DRAGON': ModelSpec(lambda a, d: _at(M.DRAGON, 'user_graph_path', a.data_root, a.data_path, 'user_graph_dict.npy')(
        *d[:6], a.dim_E, a.feature_embed, a.reg_weight, a.n_layers, a.ii_topk, a.uu_topk, a.lambda_coeff, a.aggr_mode, d.device), features=True, pre_epoch=True),
    # (main.py:280) the model DRAGON derives from: the same graph, its aggregation fused with the modality mix and the item rows
    'DualGNN': ModelSpec(lambda a, d: _at(M.DualGNN, 'user_graph_path', a.data_root, a.data_path, 'user_graph_dict.npy')(
        *d[:6], a.dim_E, a.feature_embed, a.reg_weight, a.uu_topk, a.aggr_mode, d.device), features=True, pre_epoch=True),
    # (main.py:381-383) the reference's default model: three modality tables side by side over the same user graph
    # (k = 40 hard-coded), a chunked backward; mm_image_weight comes from Model_YAML/COHESION.yaml
    'COHESION': ModelSpec(lambda a, d: _at(M.COHESION, 'user_graph_path', a.data_root, a.data_path, 'user_graph_dict.npy')(
        *d[:6], a.dim_E, a.reg_weight, a.dropout, a.n_layers, a.mm_layers, a.ii_topk, a.mm_image_weight, d.device), features=True, pre_epoch=True),
    # (main.py:321-322) three modality GCNs into a product of experts: the conv epilogue and the PoE / KL / BPR tail are
    # one launch and one autograd node, csrc/mvgae.hip
    'MVGAE': ModelSpec(lambda a, d: M.MVGAE(*d[:6], a.dim_E, a.reg_weight, a.n_layers, d.device), features=True),
    # (main.py:360-362) the graph half through the adapter; the diffusion half -- noised history rows, the denoiser's output
    # layer with both losses and its gradient in one pass -- on kernels of its own, csrc/diffmm.hip
    # not captured: three phases per epoch, the graphs its loss() multiplies with are rebuilt in the second
    'DiffMM': ModelSpec(lambda a, d: M.DiffMM(*d[:6], a.dim_E, a.reg_weight, a.n_layers, a.ssl_alpha, a.ssl_temp, a.ris_lambda, a.e_loss, a.rebuild_k,
                                             d.device), features=True, capture=False, epoch=epochs._train_epoch_diffmm),
    # (main.py:365-367) AdaGCL's vgae generator three times over -- ID, visual, textual -- on a FREEDOM-style item graph: the
    # three views of a step from one fused node (the MLP per undirected pair, weighted row sums, values), csrc/grade.hip;
    # not captured: four optimizers per batch (train_and_evaluate.py:259-284), its own loop
    'Grade': ModelSpec(lambda a, d: M.Grade(*d[:6], a.dim_E, a.reg_weight, a.n_layers, a.ssl_temp, a.ssl_alpha, a.ssl_temp2, a.noise_alpha, d.device),
                       features=True, capture=False, epoch=epochs._train_epoch_grade),
    # (main.py:327-328) two learned view generators over one fixed structure: the edge gate from two per-node scores and
    # the per-edge keep MLP on the f32 MFMA pipe, csrc/adagcl.hip; not captured: three optimizers per batch
    # (train_and_evaluate.py:72-97), its own loop
    'AdaGCL': ModelSpec(lambda a, d: M.AdaGCL(*d[:4], a.dim_E, a.reg_weight, a.n_layers, a.ssl_temp, a.ssl_alpha, d.device),
                        capture=False, epoch=epochs._train_epoch_adagcl),
    # (main.py:339-341) a learned view sampler over the fixed structure plus 100 000 random entries per step: the per-edge
    # sampler and the contrastive terms' whole-table log-sum-exp on kernels of their own, csrc/graphaug.hip
    # not captured: its views' structure -- the random entries -- changes every step; the plain loss() loop
    'GraphAug': ModelSpec(lambda a, d: M.GraphAug(*d[:4], a.dim_E, a.reg_weight, a.n_layers, a.ssl_temp, a.ssl_alpha, d.device), capture=False),
    # (main.py:374-376) two hypergraphs rebuilt every epoch from denoised hyperedge rows; the hypergraph attention layer with
    # its residual and dropout is one autograd node, csrc/mhrec.hip; three phases per epoch (train_and_evaluate.py:331-512):
    # not captured, the hypergraphs its loss() reads are rebuilt in the second
    # (Model/MHRec.py:578, :604-612 read user_graph_dict.npy and the hyperedge files under data_dir)
    'MHRec': ModelSpec(lambda a, d: _at(M.MHRec, 'data_dir', a.data_root, a.data_path)(
        *d[:6], a.dim_E, a.reg_weight, a.ii_topk, a.uu_topk, a.num_hypernodes, a.n_layers, a.h_layers, a.ssl_temp, a.ssl_alpha, a.beta1, a.beta2,
        d.device), features=True, capture=False, epoch=epochs._train_epoch_mhrec),
    # (main.py:368-369) the one model that trains nothing (train_and_evaluate.py:531-552): an item-item filter built once, every
    # user's history row blurred, sharpened and ranked, csrc/bspm.hip.  No parameter, so no optimizer.
    # The reference passes args.K_s where T_b belongs; neither is read, T_b it is here
    'BSPM': ModelSpec(lambda a, d: M.BSPM(*d[:4], a.K_s, a.T_s, a.K_b, a.T_b, a.idl_beta, d.device), trains=False, main_optimizer=False),
    # (main.py:372-373) the cross-attention denoiser: its rows come from the history CSR, its attention is csrc/cfdiff.hip
    # not captured: user-id batches, an AdamW of its own over CAM_AE (train_and_evaluate.py:317), host-sampled timesteps
    'CF_Diff': ModelSpec(lambda a, d: M.CF_Diff(d.num_user, d.num_item, d.user_item_dict, a.noise_scale, a.noise_min, a.noise_max, a.steps,
                                               a.learning_rate, d.device, seed=a.seed), capture=False, epoch=epochs._train_epoch_cfdiff, main_optimizer=False),
}


def spec_of(name):
    """The row of a registered name; for any other (the stand-in models of tests and tools) the generic case."""
    return MODELS.get(name) or ModelSpec(build=None)
