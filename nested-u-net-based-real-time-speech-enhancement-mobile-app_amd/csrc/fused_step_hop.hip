// Hop build of the one-stream frame-step kernel: the same source as fused_step.hip with the STFT analysis of the new PCM hop in front of
// op 0 and the inverse STFT / overlap-add behind the last op (FZ_HOP) -- PCM hop in, PCM hop out in ONE launch (nutls_set_hop_fusion).
#define FZ_HOP 1
#include "fused_step.hip"
