from .chunk_evenly import chunk_evenly
