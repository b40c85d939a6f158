// 4-wave LayerNormalization pipeline instantiations, 2 tiles per wave (see kernels_w4ln.inc).
#define GO2PI_W4_TPW 2
#include "kernels_w4ln.inc"
