"""A short scored generation for a kernel trace: 64 pages of a one-layer model at the full vocabulary decode 32 steps with top_n 8, so one
`rocprofv3 --kernel-trace --stats` run shows logprobs_chunk_kernel + logprobs_merge_kernel beside pick_kernel over the same rows."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from callireader_amd import synthetic
from callireader_amd.config import ModelDims
from callireader_amd.modeling_internvl_chat import InternVLChatModel

dims = ModelDims.reduced(vit_layers=1, llm_layers=1, rs_depth=1)
m = InternVLChatModel.from_state_dict(synthetic.make_state_dict(dims, seed=0), dims, max_tokens=512, max_pages=64)
g = torch.Generator().manual_seed(1)
for P in (64,):
    pages = [m.engine.embed_splice(torch.randint(0, 9000, (64,), generator=g)) for _ in range(P)]
    m.generate_pages(pages, max_new_tokens=33, eos_token_id=None, repetition_penalty=1.5, logprobs=8)
torch.cuda.synchronize()
m.close()
