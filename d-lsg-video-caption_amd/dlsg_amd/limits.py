"""The shapes the fused kernels take, as pure expressions (no import: the host tests' emulation uses them without the library).

Each function restates the argument check of one launcher in csrc/; dlsg_amd/hip.py (HipOps.*_supported) and tests/emul_ops.py
both answer from here, so the engine takes the same branch on the device and in the host schedule tests, and
tests/test_gpu_limits.py holds every function against the status its launcher returns on a grid around each limit.  The
persistent BiLSTM and the critic's lstm_seq are not here: their limits depend on the device (co-resident workgroups) and the
library answers for them itself (dlsg_bilstm_supported, dlsg_lstm_seq_supported)."""

PSL_MAX_T = 32                      # csrc/graphcore.hip: PSL_MAXT, rows of the logits tile in LDS
PSL_MAX_P = 32                      # PSL_MAXP
PSL_BWD_MAX_P = 8                   # PB_MAXP: proposals the backward keeps in registers
PSL_MAX_H = 2048                    # two columns per thread of a 1024-thread workgroup
PSL_FWD_LDS_BYTES = 64 * 1024       # theta (P x H) is what the forward stages in LDS
PSL_BWD_LDS_BYTES = 150 * 1024      # the backward stages the clip's frame nodes and du: (T + PB_MAXP) x H
SA_MAX_T = 32                       # one 32 x 32 score tile per clip
O2V_MAX_T = 32
O2V_WIDTHS = (64, 512, 1024)        # csrc/o2v16.hip is instantiated for these
DEC_TAIL_SAMPLE_MAX_WEIGHTS = 1 << 21


def o2v(T, H):
    """dlsg_o2v_fwd_multi / dlsg_o2v_bwd_multi (csrc/attention.hip)"""
    return 1 <= T <= O2V_MAX_T and H in O2V_WIDTHS


def latent_psl(T, P, H):
    """dlsg_latent_psl_fwd_multi: no limit on T x H, the frame nodes are read from memory"""
    return 1 <= T <= PSL_MAX_T and 1 <= P <= PSL_MAX_P and 4 <= H <= PSL_MAX_H and H % 4 == 0 and P * H * 4 <= PSL_FWD_LDS_BYTES


def latent_psl_bwd(T, P, H):
    """dlsg_latent_psl_bwd_multi"""
    return 1 <= T <= PSL_MAX_T and 1 <= P <= PSL_BWD_MAX_P and 4 <= H <= PSL_MAX_H and H % 4 == 0 and \
        (T + PSL_BWD_MAX_P) * H * 4 <= PSL_BWD_LDS_BYTES


def sa_core(T, D):
    """dlsg_sa_core_fwd / dlsg_sa_core_bwd"""
    return 1 <= T <= SA_MAX_T and D >= 64 and D % 64 == 0


def dec_tail_sample(V, D):
    """vocabulary x width up to which a workgroup of the word step projects its own row (HipOps.dec_tail_fwd sample=)"""
    return V * D <= DEC_TAIL_SAMPLE_MAX_WEIGHTS
