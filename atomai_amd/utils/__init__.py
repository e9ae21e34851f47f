from .coords import (cluster_coord, cluster_coord_frames, compare_coordinates, find_coord_clusters, gaussian_2d,
                     get_intensities, get_intensities_, get_nn_distances, get_nn_distances_, grid2xy, imcoordgrid,
                     map_bonds, peak_refinement, remove_edge_coord, transform_coordinates)
from .graphx import (Graph, filter_subgraphs, filter_subgraphs_, find_cycle_clusters, find_cycles, find_cycles_frames,
                     get_interatomic_r)
from .imgen import (MakeAtom, create_atom_mask_pair, create_lattice_mask, create_multiclass_lattice_mask,
                    create_multiclass_lattice_mask_)
from .img import (crop_borders, extract_patches, extract_patches_, extract_random_subimages, extract_subimages,
                  get_coord_grid, get_imgstack, imcrop_randcoord, imcrop_randpx, img_pad, img_resize)
from .nn import (Hook, average_weights, get_downsample_factor, get_nb_classes, gpu_usage_map, mock_forward,
                 reset_bnorm, sample_weights, set_train_rng, weights_init)
from .preproc import (array2list, array2list_, check_image_dims, check_signal_dims, get_array_memsize, init_dataloaders,
                      init_fcnn_dataloaders, init_imspec_dataloaders, num_classes_from_labels, preprocess_denoiser_data,
                      preprocess_training_image_data, preprocess_training_image_data_, preprocess_training_imspec_data,
                      preprocess_training_imspec_data_, to_onehot, torch_format_image, torch_format_spectra)

__all__ = [n for n in dir() if not n.startswith("_")]
