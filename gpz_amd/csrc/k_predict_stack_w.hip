// k_stack_tile_w / launch_stack_tile_w: k_predict_stack.hip's tile kernel with a width^2 per (column-output, row) read from an array, for
// the stacks of rows with input noise (gpz_predictor_stack_noisy).  The text is shared; see the head of that file.
#define GPZ_STACK_WIDTHS
#include "k_predict_stack.hip"
