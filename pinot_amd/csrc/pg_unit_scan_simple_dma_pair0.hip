// Instantiates one third of scan_simple_dma_pair_kernel<FB, VB, kAux>'s instances -- see pg_scan_simple_dma_pair_part.h.
#define PG_DMA_PAIR_PART 0
#include "pg_scan_simple_dma_pair_part.h"
