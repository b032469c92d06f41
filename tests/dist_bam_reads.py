"""One rank of `select_db` on a BAM reads file under torch.distributed.run (launched by tests/test_gpu_bam_reads.py): rank 0 decodes
the BAM on the GPU and scatters record-aligned shares of the reads; rank 0 writes the CSV.  Arguments: select_db's command line."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from metalign_amd import select_db  # noqa: E402

if __name__ == "__main__":
    select_db.select_main(select_db.select_parseargs(sys.argv[1:]))
