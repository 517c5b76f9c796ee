// Hop build of the two-stream packed kernel (plan fused_plan_lstm_g2.inc): fused_step_g2.hip with the front and back end of fused_step_hop.hip --
// waves 0 and 1 transform the two stream slots of the workgroup.
#define FZ_HOP 1
#define FZ_STREAMS 2
#include "fused_step.hip"
